// Heat-map losses: plain MSE, joint-weighted MSE with hard-keypoint mining, and the integral-regression coordinate loss.
#include <cmath>
#include "common.h"
#include "heatmap_reduce.h"

constexpr int MSE_BLOCKS = 512;

__global__ __launch_bounds__(256) void mse_partial_kernel(const float* pred, const float* target, long numel, float* grad,
                                                         const float* grad_scale, double* partial) {
    __shared__ double red[4];
    const float gs = (grad_scale ? *grad_scale : 1.f) / (float)numel;
    double acc = 0.0;
    const long nvec = numel / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const float4 p = reinterpret_cast<const float4*>(pred)[i];
        const float4 t = reinterpret_cast<const float4*>(target)[i];
        const float4 d = {p.x - t.x, p.y - t.y, p.z - t.z, p.w - t.w};
        acc += (double)(d.x * d.x) + (double)(d.y * d.y) + (double)(d.z * d.z) + (double)(d.w * d.w);
        if (grad) reinterpret_cast<float4*>(grad)[i] = float4{d.x * gs, d.y * gs, d.z * gs, d.w * gs};
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < numel; i += 256) {
            const float d = pred[i] - target[i];
            acc += (double)(d * d);
            if (grad) grad[i] = d * gs;
        }
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// loss = 0.5 * sum of the partial sums / numel: the last launch of lh_mse_heatmap and of lh_joints_mse without mining
__global__ void mse_final_kernel(const double* partial, int nblocks, long numel, float* loss) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) acc += partial[i];
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) *loss = (float)(0.5 * sum / (double)numel);
}

extern "C" size_t lh_mse_workspace_bytes(long numel) { (void)numel; return MSE_BLOCKS * sizeof(double); }

extern "C" int lh_mse_heatmap(const float* pred, const float* target, long numel, float* loss, float* grad,
                              const float* grad_scale, void* workspace, void* stream) {
    LH_REQUIRE(pred && target && loss && workspace && numel > 0, "lh_mse_heatmap: bad arguments");
    LH_REQUIRE(((uintptr_t)pred % 16 == 0) && ((uintptr_t)target % 16 == 0) && (!grad || (uintptr_t)grad % 16 == 0),
               "lh_mse_heatmap: buffers must be 16-byte aligned");
    int blocks = (int)((numel / 4 + 255) / 256);
    if (blocks > MSE_BLOCKS) blocks = MSE_BLOCKS;
    if (blocks < 1) blocks = 1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mse_partial_kernel, dim3(blocks), dim3(256), 0, s, pred, target, numel, grad, grad_scale,
                       (double*)workspace);
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, s, (const double*)workspace, blocks, numel, loss);
    LH_LAUNCH_CHECK("mse launch");
    return LH_OK;
}

// ---- JointsMSELoss(use_target_weight=True) and JointsOHKMMSELoss of the SimpleBaseline / HRNet code line (lh_joints_mse).
// One workgroup per joint plane: the plane's sum S = w^2 * sum (float)(d * d) in fp64, in a fixed order (block_sum).  Without
// mining the gradient coefficient w * w * gs is known before any sum, so the same pass writes the gradient (GRAD); with mining
// the pass only sums, joints_ohkm_select_kernel picks the planes and joints_ohkm_grad_kernel writes them.
template <bool GRAD>
__global__ __launch_bounds__(256) void joints_mse_plane_kernel(const float* pred, const float* target, const float* weight, int hw,
                                                              long numel, float* grad, const float* grad_scale, double* plane_sum,
                                                              float* joint_loss) {
    __shared__ double red[4];
    const long base = (long)blockIdx.x * hw;
    const float w = weight ? weight[blockIdx.x] : 1.f;
    float coef = 0.f;
    if (GRAD) {
        const float gs = (grad_scale ? *grad_scale : 1.f) / (float)numel;
        coef = w * w * gs;
    }
    const float4* p4 = reinterpret_cast<const float4*>(pred + base);
    const float4* t4 = reinterpret_cast<const float4*>(target + base);
    double acc = 0.0;
    for (int i = threadIdx.x; i < hw / 4; i += 256) {
        const float4 p = p4[i], t = t4[i];
        const float4 d = {p.x - t.x, p.y - t.y, p.z - t.z, p.w - t.w};
        acc += (double)(d.x * d.x) + (double)(d.y * d.y) + (double)(d.z * d.z) + (double)(d.w * d.w);
        if (GRAD) reinterpret_cast<float4*>(grad + base)[i] = float4{d.x * coef, d.y * coef, d.z * coef, d.w * coef};
    }
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const double s = (double)w * (double)w * sum;
        plane_sum[blockIdx.x] = s;
        if (joint_loss) joint_loss[blockIdx.x] = (float)(0.5 * s / (double)hw);
    }
}

// true when joint k (loss a) is picked before joint i (loss b): larger loss first, the lower joint index among equals; a NaN
// loss ranks first (lh_heatmap_argmax's rule), so it reaches the loss value instead of hiding behind the selection
__device__ __forceinline__ bool ohkm_before(float a, int k, float b, int i) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || k < i);
    return a > b || (a == b && k < i);
}

// One workgroup, thread t owns planes t, t + 256, ...: the rank of the plane's joint among its sample's fp32 per-joint losses
// (j comparisons), the coefficient w * w * gs_k and the selection flag for the gradient pass, and
// loss = (1/b) sum_b (1/topk) sum_selected 0.5 * S / hw accumulated in fp64 in a fixed order.
__global__ __launch_bounds__(256) void joints_ohkm_select_kernel(const double* plane_sum, const float* weight, int b, int j, int hw,
                                                                int topk, const float* grad_scale, float* coef, int* selected,
                                                                float* loss) {
    __shared__ double red[4];
    const float gs = (grad_scale ? *grad_scale : 1.f) / (float)((long)b * topk * hw);
    double acc = 0.0;
    for (int idx = threadIdx.x; idx < b * j; idx += 256) {
        const int i = idx % j;
        const double* ps = plane_sum + (idx - i);
        const double li = 0.5 * ps[i] / (double)hw;
        const float fi = (float)li;
        int rank = 0;
        for (int k = 0; k < j; ++k)
            if (k != i && ohkm_before((float)(0.5 * ps[k] / (double)hw), k, fi, i)) ++rank;
        const bool sel = rank < topk;
        const float w = weight ? weight[idx] : 1.f;
        coef[idx] = sel ? w * w * gs : 0.f;
        selected[idx] = sel ? 1 : 0;
        if (sel) acc += li;
    }
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) *loss = (float)(sum / ((double)b * (double)topk));
}

// planes that were not selected are not read: their gradient is exactly 0.f
__global__ __launch_bounds__(256) void joints_ohkm_grad_kernel(const float* pred, const float* target, int hw, const float* coef,
                                                              const int* selected, float* grad) {
    const long base = (long)blockIdx.x * hw;
    float4* g4 = reinterpret_cast<float4*>(grad + base);
    if (!selected[blockIdx.x]) {
        for (int i = threadIdx.x; i < hw / 4; i += 256) g4[i] = float4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const float c = coef[blockIdx.x];
    const float4* p4 = reinterpret_cast<const float4*>(pred + base);
    const float4* t4 = reinterpret_cast<const float4*>(target + base);
    for (int i = threadIdx.x; i < hw / 4; i += 256) {
        const float4 p = p4[i], t = t4[i];
        g4[i] = float4{(p.x - t.x) * c, (p.y - t.y) * c, (p.z - t.z) * c, (p.w - t.w) * c};
    }
}

// workspace: fp64 plane sums [b][j], then the fp32 coefficient table and the int32 selection flags of the mining pass
extern "C" size_t lh_joints_mse_workspace_bytes(int b, int j) {
    return b > 0 && j > 0 ? (size_t)b * j * (sizeof(double) + sizeof(float) + sizeof(int)) : 0;
}

extern "C" int lh_joints_mse(const float* pred, const float* target, const float* weight, int b, int j, int hw, int topk, float* loss,
                             float* joint_loss, float* grad, const float* grad_scale, void* workspace, void* stream) {
    LH_REQUIRE(pred && target && loss && workspace && b > 0 && j > 0 && hw > 0, "lh_joints_mse: bad arguments");
    LH_REQUIRE(topk >= 0 && topk <= j, "lh_joints_mse: topk %d outside 0..%d (the joints of a sample)", topk, j);
    LH_REQUIRE(hw % 4 == 0, "lh_joints_mse: the plane size %d must be a multiple of 4", hw);
    LH_REQUIRE((long)b * j < (1L << 31), "lh_joints_mse: too many planes");
    LH_REQUIRE(((uintptr_t)pred % 16 == 0) && ((uintptr_t)target % 16 == 0) && (!grad || (uintptr_t)grad % 16 == 0) &&
               ((uintptr_t)workspace % 16 == 0), "lh_joints_mse: buffers must be 16-byte aligned");
    const int bj = b * j;
    const long numel = (long)bj * hw;
    double* plane_sum = (double*)workspace;
    float* coef = (float*)(plane_sum + bj);
    int* selected = (int*)(coef + bj);
    hipStream_t s = (hipStream_t)stream;
    if (topk == 0) {
        if (grad)
            hipLaunchKernelGGL((joints_mse_plane_kernel<true>), dim3(bj), dim3(256), 0, s, pred, target, weight, hw, numel, grad,
                               grad_scale, plane_sum, joint_loss);
        else
            hipLaunchKernelGGL((joints_mse_plane_kernel<false>), dim3(bj), dim3(256), 0, s, pred, target, weight, hw, numel,
                               (float*)nullptr, grad_scale, plane_sum, joint_loss);
        hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, s, (const double*)plane_sum, bj, numel, loss);
        LH_LAUNCH_CHECK("joints_mse launch");
        return LH_OK;
    }
    hipLaunchKernelGGL((joints_mse_plane_kernel<false>), dim3(bj), dim3(256), 0, s, pred, target, weight, hw, numel, (float*)nullptr,
                       grad_scale, plane_sum, joint_loss);
    hipLaunchKernelGGL(joints_ohkm_select_kernel, dim3(1), dim3(256), 0, s, (const double*)plane_sum, weight, b, j, hw, topk, grad_scale,
                       coef, selected, loss);
    if (grad)
        hipLaunchKernelGGL(joints_ohkm_grad_kernel, dim3(bj), dim3(256), 0, s, pred, target, hw, (const float*)coef, (const int*)selected,
                           grad);
    LH_LAUNCH_CHECK("joints_ohkm launch");
    return LH_OK;
}

// ---- Integral-regression coordinate loss (Sun et al. 2018, "Integral Human Pose Regression"; an opt-in extension without a
// reference oracle): L1 between the soft-arg-max of a plane and its ground-truth joint, and the gradient of that through the
// softmax, added to the heat-map loss's outputs (lh_integral_l1).  One workgroup per plane:
//   1. the plane goes to LDS (h*w floats, sized by the launch: 16 KB for a 64 x 64 plane) with 16-byte loads, the maximum is
//      taken on the way;
//   2. e_p = expf(beta * (hm_p - max)) replaces the plane in LDS; S0, sum e x, sum e y in fp64 with the thread stride of
//      heatmap_soft_argmax_kernel and the block reductions it uses, so preds has that kernel's bits;
//   3. every thread forms the expectation, the residual's signs and k_n from the sums, thread 0 stores preds and the plane's
//      loss; the gradient pass reads e_p from LDS and reads / writes grad with 16-byte accesses.
// A plane of weight 0 skips pass 3's gradient (accumulate) or stores zeros (write).  No atomics: two calls give the same bits.
constexpr int INTEGRAL_MAX_HW = 96 * 96;
constexpr size_t INTEGRAL_WS_HEAD = 16;                   // workspace: fp32 loss_c (+ padding), then the fp64 plane losses

__device__ __forceinline__ float sgnf(float r) { return r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void integral_l1_kernel(const float* hm, const float* joints, int jstride, const float* weight, int bj,
                                                         int hw, int w, float beta, float scale, float lambda, float* preds,
                                                         float* joint_loss, double* plane_loss, float* grad, int add_to_grad,
                                                         const float* grad_scale) {
    extern __shared__ __attribute__((aligned(16))) float plane[];      // hw floats, sized by the launch
    __shared__ float rmax[4];
    __shared__ double rs[4][3];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float4* m4 = reinterpret_cast<const float4*>(hm + (long)n * hw);
    float mx = -INFINITY;
    for (int i = tid; i < hw / 4; i += 256) {
        const float4 v = m4[i];
        reinterpret_cast<float4*>(plane)[i] = v;
        mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
    }
    mx = block_max(mx, rmax);
    double s0 = 0.0, sx = 0.0, sy = 0.0;
    for (int i = tid; i < hw; i += 256) {                  // element i is read and replaced by this thread only
        const float ef = expf(beta * (plane[i] - mx));
        plane[i] = ef;
        const double e = (double)ef;
        s0 += e; sx += e * (double)(i % w); sy += e * (double)(i / w);
    }
    const Moments t = block_sum_moments(s0, sx, sy, rs);
    const double t0 = t.s0, ex = t.sx / t0, ey = t.sy / t0;
    const float px = (float)ex * scale, py = (float)ey * scale;
    const float rx = px - joints[(long)n * jstride], ry = py - joints[(long)n * jstride + 1];
    const float wgt = weight ? weight[n] : 1.f;
    if (tid == 0) {
        preds[n * 2 + 0] = px;
        preds[n * 2 + 1] = py;
        const float jl = wgt * (fabsf(rx) + fabsf(ry));
        if (joint_loss) joint_loss[n] = jl;
        plane_loss[n] = (double)jl;
    }
    if (!grad) return;
    float4* g4 = reinterpret_cast<float4*>(grad + (long)n * hw);
    if (wgt == 0.f) {                                      // exactly 0.f: written, or nothing to add
        if (!add_to_grad)
            for (int i = tid; i < hw / 4; i += 256) g4[i] = float4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const double dsx = (double)sgnf(rx), dsy = (double)sgnf(ry);
    const double gs = grad_scale ? (double)*grad_scale : 1.0;
    const float k = (float)(gs * (double)lambda * (double)wgt * (double)scale * (double)beta / (2.0 * (double)bj) / t0);
    for (int i = tid; i < hw / 4; i += 256) {
        const float4 e = reinterpret_cast<const float4*>(plane)[i];
        const float ev[4] = {e.x, e.y, e.z, e.w};
        float g[4];
        int yc =(i * 4) / w, xc = i * 4 - yc * w;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            g[c] = (ev[c] * k) * (float)(((double)xc - ex) * dsx + ((double)yc - ey) * dsy);
            if (++xc == w) { xc = 0; ++yc; }                           // the four elements may cross a row end
        }
        if (add_to_grad) {
            const float4 o = g4[i];
            g4[i] = float4{o.x + g[0], o.y + g[1], o.z + g[2], o.w + g[3]};
        } else {
            g4[i] = float4{g[0], g[1], g[2], g[3]};
        }
    }
}

// loss_c = lambda * sum_n plane_loss[n] / (2*b*j), summed in fp64 in plane order by thread 0 (the others stage tiles of 256 in LDS)
__global__ __launch_bounds__(256) void integral_l1_fold_kernel(const double* plane_loss, int bj, float lambda, float* loss_c, float* loss,
                                                              int add_to_loss) {
    __shared__ double tile[256];
    double acc = 0.0;
    for (int base = 0; base < bj; base += 256) {
        tile[threadIdx.x] = base + (int)threadIdx.x < bj ? plane_loss[base + threadIdx.x] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = bj - base < 256 ? bj - base : 256;
            for (int k = 0; k < cnt; ++k) acc += tile[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float lc = (float)((double)lambda * acc / (2.0 * (double)bj));
        *loss_c = lc;
        *loss = add_to_loss ? *loss + lc : lc;
    }
}

extern "C" size_t lh_integral_l1_workspace_bytes(int b, int j) {
    return b > 0 && j > 0 ? INTEGRAL_WS_HEAD + (size_t)b * j * sizeof(double) : 0;
}

extern "C" int lh_integral_l1(const float* heatmaps, const float* joints, int jstride, const float* weight, int b, int j, int h, int w,
                              float beta, float scale, float lambda, float* preds, float* joint_loss, float* loss, int add_to_loss,
                              float* grad, int add_to_grad, const float* grad_scale, void* workspace, void* stream) {
    LH_REQUIRE(heatmaps && joints && preds && loss && workspace && jstride >= 2 && b > 0 && j > 0 && h > 0 && w > 0,
               "lh_integral_l1: bad arguments");
    LH_REQUIRE((long)b * j < (1L << 30), "lh_integral_l1: too many planes");
    LH_REQUIRE(beta > 0.f && std::isfinite(beta) && std::isfinite(scale) && std::isfinite(lambda),
               "lh_integral_l1: beta must be positive, beta / scale / lambda finite");
    LH_REQUIRE((long)h * w <= INTEGRAL_MAX_HW, "lh_integral_l1: a plane of %d x %d exceeds the %d elements the kernel holds in LDS", h, w,
               INTEGRAL_MAX_HW);
    LH_REQUIRE((h * w) % 4 == 0, "lh_integral_l1: the plane size %d must be a multiple of 4", h * w);
    LH_REQUIRE(((uintptr_t)heatmaps % 16 == 0) && (!grad || (uintptr_t)grad % 16 == 0) && ((uintptr_t)workspace % 16 == 0),
               "lh_integral_l1: buffers must be 16-byte aligned");
    const int bj = b * j;
    float* loss_c = (float*)workspace;
    double* plane_loss = (double*)((char*)workspace + INTEGRAL_WS_HEAD);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(integral_l1_kernel, dim3(bj), dim3(256), (size_t)h * w * sizeof(float), s, heatmaps, joints, jstride, weight, bj, h * w, w, beta, scale, lambda,
                       preds, joint_loss, plane_loss, grad, add_to_grad ? 1 : 0, grad_scale);
    hipLaunchKernelGGL(integral_l1_fold_kernel, dim3(1), dim3(256), 0, s, (const double*)plane_loss, bj, lambda, loss_c, loss,
                       add_to_loss ? 1 : 0);
    LH_LAUNCH_CHECK("integral_l1 launch");
    return LH_OK;
}
