// Heat-maps: Gaussian target renderers, MSE / weighted / hard-keypoint-mining losses, arg-max family decode, PCK / EPE metrics.
#include <cmath>
#include "common.h"

// ------------------------------------------------------------------------------------------------ Gaussian target
// generate_target (src/tools/dataset.py:171-186).  WEIGHTED renders upstream's target_weight with it (`if v > 0.5:`): weight =
// visibility x "some part of the patch lies inside the map", a joint of weight 0 gets a zero map, and the thread that owns pixel
// (0, 0) of a plane writes that plane's weight.  A compile-time switch: the unweighted instantiation never reads vis / weight
// (passed as null) and keeps the resource table it had as a kernel of its own (tools/kres.py).
// SUB (lh_gaussian_target_sub, DARK's unbiased encoding): the same window, skip test and weight, but the value inside the window
// is the Gaussian around the joint's real-valued heat-map position, one expf per pixel; `patch` is not read.  A second
// compile-time switch, so the two quantised instantiations keep their code.
template <bool WEIGHTED, bool SUB = false>
__global__ void gaussian_target_kernel(const float* joints, int jstride, const float* vis, int vstride, const float* patch,
                                       int radius, float* target, float* weight, int bj, int size, float sigma) {
    const long total = (long)bj * size * size;
    const int pw = 2 * radius + 1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % size);
        const long t = i / size;
        const int y = (int)(t % size);
        const long j = t / size;
        const float jx = joints[j * jstride], jy = joints[j * jstride + 1];
        // int(v / 4 + 0.5): truncation toward zero, like Python's int()
        const int mx = (int)(jx * 0.25f + 0.5f), my = (int)(jy * 0.25f + 0.5f);
        const int x0 = mx - radius, y0 = my - radius, x1 = mx + radius + 1, y1 = my + radius + 1;
        const bool skip = x0 >= size || y0 >= size || x1 < 0 || y1 < 0;
        bool draw = !skip;
        float w = 0.f;
        if constexpr (WEIGHTED) {
            const float v = vis ? vis[j * vstride] : 1.f;
            w = (v > 0.5f ? v : 0.f) * (skip ? 0.f : 1.f);
            draw = w > 0.f;
        }
        float out = 0.f;
        if (draw && x >= x0 && x < x1 && y >= y0 && y < y1) {
            if constexpr (SUB) {
                const float dx = (float)x - jx * 0.25f, dy = (float)y - jy * 0.25f;
                out = expf(-(dx * dx + dy * dy) / (2.f * sigma * sigma));
            } else {
                out = patch[(y - y0) * pw + (x - x0)];
            }
        }
        target[i] = out;
        if constexpr (WEIGHTED)
            if (x == 0 && y == 0) weight[j] = w;
    }
}

// GenerateHeatmap (src/utils/dataset_loader.py:22-53), the alternate renderer: points are ALREADY in heat-map coordinates,
// sigma = res / 64 (an integer here), patch of (6 * sigma + 3)^2 centred on int(point), np.maximum blend with the zero
// map (= plain placement: every joint owns its plane); a joint is skipped when x <= 0 or int(point) lies outside the map.
__global__ void gaussian_target_alt_kernel(const float* points, int pstride, const float* patch, int sigma, float* target,
                                           int bj, int res) {
    const long total = (long)bj * res * res;
    const int pw = 6 * sigma + 3;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % res);
        const long t = i / res;
        const int y = (int)(t % res);
        const long j = t / res;
        const float fx = points[j * pstride], fy = points[j * pstride + 1];
        float v = 0.f;
        if (fx > 0.f) {
            const int px = (int)fx, py = (int)fy;                    // Python int(): truncation toward zero
            if (px >= 0 && py >= 0 && px < res && py < res) {
                const int ulx = px - 3 * sigma - 1, uly = py - 3 * sigma - 1;
                const int gx = x - ulx, gy = y - uly;                // hms[aa:bb, cc:dd] <- g[a:b, c:d]: same offset on both axes
                if (gx >= 0 && gx < pw && gy >= 0 && gy < pw) v = patch[gy * pw + gx];
            }
        }
        target[i] = v;
    }
}

extern "C" int lh_gaussian_target_alt(const float* points, int pstride, const float* patch, int sigma, float* target,
                                      int b, int j, int res, void* stream) {
    LH_REQUIRE(points && patch && target && pstride >= 2 && b > 0 && j > 0 && res > 0 && sigma >= 1 && res == 64 * sigma,
               "lh_gaussian_target_alt: bad arguments (res must be 64 * sigma, sigma a positive integer)");
    const long total = (long)b * j * res * res;
    const int grid = lh_grid(total, 4096);
    hipLaunchKernelGGL(gaussian_target_alt_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, points, pstride, patch, sigma,
                       target, b * j, res);
    LH_LAUNCH_CHECK("gaussian_target_alt launch");
    return LH_OK;
}

extern "C" int lh_gaussian_target(const float* joints, int jstride, const float* patch, int radius, float* target,
                                  int b, int j, int size, void* stream) {
    LH_REQUIRE(joints && patch && target && jstride >= 2 && b > 0 && j > 0 && size > 0 && radius >= 0,
               "lh_gaussian_target: bad arguments");
    hipLaunchKernelGGL(gaussian_target_kernel<false>, dim3(lh_grid((long)b * j * size * size, 4096)), dim3(256), 0, (hipStream_t)stream,
                       joints, jstride, (const float*)nullptr, 0, patch, radius, target, (float*)nullptr, b * j, size, 0.f);
    LH_LAUNCH_CHECK("gaussian_target launch");
    return LH_OK;
}

extern "C" int lh_gaussian_target_w(const float* joints, int jstride, const float* vis, int vstride, const float* patch, int radius,
                                    float* target, float* weight, int b, int j, int size, void* stream) {
    LH_REQUIRE(joints && patch && target && weight && jstride >= 2 && (!vis || vstride >= 1) && b > 0 && j > 0 && size > 0 && radius >= 0,
               "lh_gaussian_target_w: bad arguments");
    hipLaunchKernelGGL(gaussian_target_kernel<true>, dim3(lh_grid((long)b * j * size * size, 4096)), dim3(256), 0, (hipStream_t)stream,
                       joints, jstride, vis, vstride, patch, radius, target, weight, b * j, size, 0.f);
    LH_LAUNCH_CHECK("gaussian_target_w launch");
    return LH_OK;
}

extern "C" int lh_gaussian_target_sub(const float* joints, int jstride, const float* vis, int vstride, int radius, float sigma,
                                      float* target, float* weight, int b, int j, int size, void* stream) {
    LH_REQUIRE(joints && target && jstride >= 2 && (!vis || vstride >= 1) && b > 0 && j > 0 && size > 0 && radius >= 0 && sigma > 0.f,
               "lh_gaussian_target_sub: bad arguments (sigma must be positive)");
    const dim3 grid(lh_grid((long)b * j * size * size, 4096));
    if (weight)
        hipLaunchKernelGGL((gaussian_target_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, joints, jstride, vis, vstride,
                           (const float*)nullptr, radius, target, weight, b * j, size, sigma);
    else
        hipLaunchKernelGGL((gaussian_target_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, joints, jstride,
                           (const float*)nullptr, 0, (const float*)nullptr, radius, target, (float*)nullptr, b * j, size, sigma);
    LH_LAUNCH_CHECK("gaussian_target_sub launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ MSE loss
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
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void mse_final_kernel(const double* partial, int nblocks, long numel, float* loss) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) acc += partial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) *loss = (float)(0.5 * (red[0] + red[1] + red[2] + red[3]) / (double)numel);
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
// One workgroup per joint plane: the plane's sum S = w^2 * sum (float)(d * d) in fp64, in a fixed order (the reduction of
// mse_partial_kernel: per-thread fp64 accumulator, wave-64 shuffle, four LDS slots; no atomics, so every replay gives the same
// bits).  Without mining the gradient coefficient w * w * gs is known before any sum, so the same pass writes the gradient
// (GRAD); with mining the pass only sums, joints_ohkm_select_kernel picks the planes and joints_ohkm_grad_kernel writes them.
__device__ __forceinline__ double plane_reduce(double acc, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

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
    const double sum = plane_reduce(acc, red);
    if (threadIdx.x == 0) {
        const double s = (double)w * (double)w * sum;
        plane_sum[blockIdx.x] = s;
        if (joint_loss) joint_loss[blockIdx.x] = (float)(0.5 * s / (double)hw);
    }
}

__global__ __launch_bounds__(256) void joints_mse_final_kernel(const double* plane_sum, int bj, long numel, float* loss) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < bj; i += 256) acc += plane_sum[i];
    const double sum = plane_reduce(acc, red);
    if (threadIdx.x == 0) *loss = (float)(0.5 * sum / (double)numel);
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
    const double sum = plane_reduce(acc, red);
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
        hipLaunchKernelGGL(joints_mse_final_kernel, dim3(1), dim3(256), 0, s, (const double*)plane_sum, bj, numel, loss);
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

// ------------------------------------------------------------------------------------------------ arg-max decode
struct Cand { float v; int i; };
// true when a precedes b under numpy.argmax's rule: NaN beats everything, then larger value,
// ties (and NaN vs NaN) broken by the lower flat index.
__device__ __forceinline__ bool cand_before(const Cand& a, const Cand& b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an || bn) return an && (!bn || a.i < b.i);
    return a.v > b.v || (a.v == b.v && a.i < b.i);
}

__global__ __launch_bounds__(256) void heatmap_argmax_kernel(const float* hm, int hw, int w, float scale, float* preds,
                                                            float* maxvals, int* idx) {
    __shared__ Cand red[4];
    const float* m = hm + (long)blockIdx.x * hw;
    Cand best = {0.f, 0x7fffffff};
    bool have = false;
    for (int i = threadIdx.x; i < hw; i += 256) {
        const Cand c = {m[i], i};
        if (!have || cand_before(c, best)) { best = c; have = true; }
    }
    if (!have) best = Cand{-INFINITY, 0x7fffffff};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand other = {__shfl_xor(best.v, o), __shfl_xor(best.i, o)};
        if (other.i != 0x7fffffff && (best.i == 0x7fffffff || cand_before(other, best))) best = other;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        Cand b = red[0];
        for (int k = 1; k < 4; ++k)
            if (red[k].i != 0x7fffffff && (b.i == 0x7fffffff || cand_before(red[k], b))) b = red[k];
        const float keep = b.v > 0.f ? 1.f : 0.f;
        preds[blockIdx.x * 2 + 0] = (float)(b.i % w) * keep * scale;
        preds[blockIdx.x * 2 + 1] = (float)(b.i / w) * keep * scale;
        maxvals[blockIdx.x] = b.v;
        if (idx) idx[blockIdx.x] = b.i;
    }
}

extern "C" int lh_heatmap_argmax(const float* heatmaps, int bj, int h, int w, float scale, float* preds, float* maxvals,
                                 int* idx, void* stream) {
    LH_REQUIRE(heatmaps && preds && maxvals && bj > 0 && h > 0 && w > 0, "lh_heatmap_argmax: bad arguments");
    hipLaunchKernelGGL(heatmap_argmax_kernel, dim3(bj), dim3(256), 0, (hipStream_t)stream, heatmaps, h * w, w, scale, preds,
                       maxvals, idx);
    LH_LAUNCH_CHECK("heatmap_argmax launch");
    return LH_OK;
}

// Opt-in quarter-pixel refinement of the hard arg-max (the reference carries the switch
// TEST.POST_PROCESS, src/modeling/simplebaseline/config.py:109, but never uses it): the published SimpleBaseline
// `get_final_preds` rule -- when the peak (px, py) is strictly inside the map (1 < px < W-1, 1 < py < H-1) move it a
// quarter pixel toward the higher neighbour on each axis: coord += 0.25 * sign(hm[..+1] - hm[..-1]).  Works on the
// UNSCALED peak; `scale` is the factor lh_heatmap_argmax already applied to `preds`.
__global__ void heatmap_refine_kernel(const float* hm, const int* idx, const float* maxvals, int bj, int h, int w,
                                      float scale, float* preds) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= bj) return;
    if (!(maxvals[t] > 0.f)) return;                      // get_max_preds zeroed the coordinate: px = py = 0, never interior
    const int k = idx[t];
    const int px = k % w, py = k / w;
    if (!(1 < px && px < w - 1 && 1 < py && py < h - 1)) return;
    const float* m = hm + (long)t * h * w;
    const float dx = m[py * w + px + 1] - m[py * w + px - 1];
    const float dy = m[(py + 1) * w + px] - m[(py - 1) * w + px];
    const float sx = dx > 0.f ? 1.f : (dx < 0.f ? -1.f : 0.f), sy = dy > 0.f ? 1.f : (dy < 0.f ? -1.f : 0.f);
    preds[t * 2 + 0] = ((float)px + 0.25f * sx) * scale;
    preds[t * 2 + 1] = ((float)py + 0.25f * sy) * scale;
}

extern "C" int lh_heatmap_refine(const float* heatmaps, const int* idx, const float* maxvals, int bj, int h, int w,
                                 float scale, float* preds, void* stream) {
    LH_REQUIRE(heatmaps && idx && maxvals && preds && bj > 0 && h > 0 && w > 0, "lh_heatmap_refine: bad arguments");
    hipLaunchKernelGGL(heatmap_refine_kernel, dim3((bj + 255) / 256), dim3(256), 0, (hipStream_t)stream, heatmaps, idx, maxvals,
                       bj, h, w, scale, preds);
    LH_LAUNCH_CHECK("heatmap_refine launch");
    return LH_OK;
}

// Opt-in DARK decode (Zhang et al. 2020, "Distribution-Aware Coordinate Representation of Keypoint": the published
// get_final_preds -> gaussian_blur -> taylor chain), the sibling of heatmap_refine_kernel.  One workgroup per plane:
//   1. the plane goes to LDS (16-byte loads where the plane base allows them);
//   2. row pass of the separable zero-padded Gaussian: every thread blurs its elements i = tid + 256 u into registers, and after
//      a barrier the registers replace the plane in LDS (one buffer: 36 KB for 96 x 96);
//   3. column pass from LDS -- a wave's lanes hold consecutive x, so the stride-w reads of one tap are conflict-free -- of
//      which only the maximum over the plane is kept (wave shuffles, four LDS slots);
//   4. threads 0..12 redo the column pass at the 13 stencil points and store C = log(max(B * maxval / max B, 1e-10)); thread 0
//      takes the derivatives and solves the 2 x 2 system.
// Taps are accumulated in index order, a tap that falls outside the plane adds nothing.  No atomics: two calls give the same
// bits.  The finiteness guard on the offset is this project's; OpenCV's fixed tap tables for kernels <= 7 are not reproduced.
constexpr int DARK_MAX_HW = 96 * 96, DARK_MAX_TAPS = 17, DARK_PER_THREAD = DARK_MAX_HW / 256;
struct DarkTaps { float g[DARK_MAX_TAPS]; };

// column pass at (x, y) of the row-blurred plane in LDS
__device__ __forceinline__ float dark_col(const float* rowb, const float* g, int k, int c, int x, int y, int h, int w) {
    float acc = 0.f;
    for (int t = 0; t < k; ++t) {
        const int yy = y + t - c;
        if (yy >= 0 && yy < h) acc += g[t] * rowb[yy * w + x];
    }
    return acc;
}

__global__ __launch_bounds__(256) void heatmap_dark_kernel(const float* hm, const int* idx, const float* maxvals, int h, int w, int k,
                                                          DarkTaps taps, int vec, float scale, float* preds) {
    __shared__ __attribute__((aligned(16))) float plane[DARK_MAX_HW];
    __shared__ float g[DARK_MAX_TAPS];
    __shared__ float red[4];
    __shared__ float cs[13];
    const int p = blockIdx.x, tid = threadIdx.x, hw = h * w, c = k >> 1;
    const float maxval = maxvals[p];
    if (!(maxval > 0.f)) return;                          // get_max_preds zeroed the coordinate (or the maximum is a NaN)
    const int peak = idx[p];
    const int px = peak % w, py = peak / w;
    if (!(1 < px && px < w - 2 && 1 < py && py < h - 2)) return;      // uniform over the workgroup: no barrier is skipped by a part of it
    const float* m = hm + (long)p * hw;
    if (tid < k) g[tid] = taps.g[tid];
    if (vec) {
        for (int i = tid; i < hw / 4; i += 256) reinterpret_cast<float4*>(plane)[i] = reinterpret_cast<const float4*>(m)[i];
    } else {
        for (int i = tid; i < hw; i += 256) plane[i] = m[i];
    }
    __syncthreads();
    float r[DARK_PER_THREAD];
#pragma unroll
    for (int u = 0; u < DARK_PER_THREAD; ++u) {
        const int i = tid + u * 256;
        r[u] = 0.f;
        if (i < hw) {
            const int y = i / w, x = i - y * w;
            float acc = 0.f;
            for (int t = 0; t < k; ++t) {
                const int xx = x + t - c;
                if (xx >= 0 && xx < w) acc += g[t] * plane[y * w + xx];
            }
            r[u] = acc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < DARK_PER_THREAD; ++u) {
        const int i = tid + u * 256;
        if (i < hw) plane[i] = r[u];
    }
    __syncthreads();
    float bmax = -INFINITY;
#pragma unroll 4
    for (int u = 0; u < DARK_PER_THREAD; ++u) {
        const int i = tid + u * 256;
        if (i < hw) {
            const int y = i / w, x = i - y * w;
            bmax = fmaxf(bmax, dark_col(plane, g, k, c, x, y, h, w));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, o));
    if ((tid & 63) == 0) red[tid >> 6] = bmax;
    __syncthreads();
    if (tid < 13) {
        // stencil points: 0..4 = (px-2 .. px+2, py), 5..8 = (px, py-2), (px, py-1), (px, py+1), (px, py+2), 9..12 = the diagonals
        // (-1,-1), (+1,-1), (-1,+1), (+1,+1); all inside the plane by the skip test
        int ox, oy;
        if (tid < 5) { ox = tid - 2; oy = 0; }
        else if (tid < 9) { ox = 0; oy = tid < 7 ? tid - 7 : tid - 6; }
        else { ox = (tid - 9) & 1 ? 1 : -1; oy = tid < 11 ? -1 : 1; }
        const float s = maxval / fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        cs[tid] = logf(fmaxf(dark_col(plane, g, k, c, px + ox, py + oy, h, w) * s, 1e-10f));
    }
    __syncthreads();
    if (tid == 0) {
        const float dx = 0.5f * (cs[3] - cs[1]), dy = 0.5f * (cs[7] - cs[6]);
        const float dxx = 0.25f * (cs[4] - 2.f * cs[2] + cs[0]), dyy = 0.25f * (cs[8] - 2.f * cs[2] + cs[5]);
        const float dxy = 0.25f * (cs[12] - cs[10] - cs[11] + cs[9]);
        const float det = dxx * dyy - dxy * dxy;
        if (det != 0.f) {
            const float offx = -(dyy * dx - dxy * dy) / det, offy = -(dxx * dy - dxy * dx) / det;
            if (isfinite(offx) && isfinite(offy)) {
                preds[p * 2 + 0] = ((float)px + offx) * scale;
                preds[p * 2 + 1] = ((float)py + offy) * scale;
            }
        }
    }
}

extern "C" int lh_heatmap_dark(const float* heatmaps, const int* idx, const float* maxvals, int bj, int h, int w, int blur_kernel,
                               float scale, float* preds, void* stream) {
    LH_REQUIRE(heatmaps && idx && maxvals && preds && bj > 0 && h > 0 && w > 0, "lh_heatmap_dark: bad arguments");
    LH_REQUIRE((long)h * w <= DARK_MAX_HW, "lh_heatmap_dark: a plane of %d x %d exceeds the %d elements the kernel holds in LDS", h, w,
               DARK_MAX_HW);
    LH_REQUIRE(blur_kernel >= 3 && blur_kernel <= DARK_MAX_TAPS && (blur_kernel & 1),
               "lh_heatmap_dark: blur_kernel %d must be odd and lie in 3..%d", blur_kernel, DARK_MAX_TAPS);
    // cv2.getGaussianKernel's formula for sigma <= 0, in fp64, normalised to sum 1 and rounded to fp32
    DarkTaps taps = {};
    double gd[DARK_MAX_TAPS], sum = 0.0;
    const double c = (blur_kernel - 1) * 0.5, sg = 0.3 * ((blur_kernel - 1) * 0.5 - 1.0) + 0.8;
    for (int t = 0; t < blur_kernel; ++t) sum += gd[t] = exp(-(t - c) * (t - c) / (2.0 * sg * sg));
    for (int t = 0; t < blur_kernel; ++t) taps.g[t] = (float)(gd[t] / sum);
    const int vec = (h * w) % 4 == 0 && (uintptr_t)heatmaps % 16 == 0;
    hipLaunchKernelGGL(heatmap_dark_kernel, dim3(bj), dim3(256), 0, (hipStream_t)stream, heatmaps, idx, maxvals, h, w, blur_kernel, taps,
                       vec, scale, preds);
    LH_LAUNCH_CHECK("heatmap_dark launch");
    return LH_OK;
}

// Flip test (TEST.FLIP_TEST / TEST.SHIFT_HEATMAP of the reference's configs) after the two forwards, in one launch: a = the
// plain pass's heat-maps, m = those of the pass on the horizontally mirrored input.  SimpleBaseline's flip_back, its
// `output_flipped[..., 1:] = output_flipped.clone()[..., :-1]` and `(output + output_flipped) * 0.5`:
//   shift:    f[y][x] = m[y][W-x] for x >= 1, f[y][0] = m[y][W-1];   no shift: f[y][x] = m[y][W-1-x]
//   merged = (a + f) * 0.5f (two fp32 roundings: -ffp-contract=off), then heatmap_argmax_kernel's decode of merged.
// No joint permutation: the 21 joints of one hand are their own mirror images.
// Why the one-column shift is right for this project's coordinates: the target of a joint at input x is centred on column
// int(x / 4 + 0.5) and the decode multiplies the peak column by 4, so a joint at x = 4k peaks at column k.  The mirrored input
// (width 4W) holds it at 4W-1-4k, centred on int(W - k + 0.25) = W - k; flipped back that is column W-1-(W-k) = k-1, and the
// shift brings it back to k.
// One workgroup per map, the tie rule of heatmap_argmax_kernel.  A thread loads a chunk of U elements of a and of m into
// registers before it stores any of them: merged may alias a (each element is read and written by the same thread only), and
// the loads of a chunk stay independent of its stores.
template <int U>
__global__ __launch_bounds__(256) void heatmap_flip_merge_kernel(const float* a, const float* m, int hw, int w, int shift, float scale,
                                                                 float* merged, float* preds, float* maxvals, int* idx) {
    __shared__ Cand red[4];
    const long base = (long)blockIdx.x * hw;
    const float* am = a + base;
    const float* mm = m + base;
    float* om = merged + base;
    const int dy = 256 / w, dx = 256 - dy * w;                // element i + 256 is dy rows and dx columns further
    Cand best = {0.f, 0x7fffffff};
    bool have = false;
    int y = threadIdx.x / w, x = threadIdx.x - y * w;          // row and column of element i0
    for (int i0 = threadIdx.x; i0 < hw; i0 += 256 * U) {
        float va[U], vf[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            va[u] = vf[u] = 0.f;
            if (i < hw) {
                const int sx = shift ? (x ? w - x : w - 1) : w - 1 - x;
                va[u] = am[i];
                vf[u] = mm[y * w + sx];
            }
            x += dx;
            y += dy;
            if (x >= w) { x -= w; ++y; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            if (i < hw) {
                const float v = (va[u] + vf[u]) * 0.5f;
                om[i] = v;
                const Cand c = {v, i};
                if (!have || cand_before(c, best)) { best = c; have = true; }
            }
        }
    }
    // the reduction and store of heatmap_argmax_kernel, restated: that kernel keeps its code
    if (!have) best = Cand{-INFINITY, 0x7fffffff};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand other = {__shfl_xor(best.v, o), __shfl_xor(best.i, o)};
        if (other.i != 0x7fffffff && (best.i == 0x7fffffff || cand_before(other, best))) best = other;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        Cand b = red[0];
        for (int k = 1; k < 4; ++k)
            if (red[k].i != 0x7fffffff && (b.i == 0x7fffffff || cand_before(red[k], b))) b = red[k];
        const float keep = b.v > 0.f ? 1.f : 0.f;
        preds[blockIdx.x * 2 + 0] = (float)(b.i % w) * keep * scale;
        preds[blockIdx.x * 2 + 1] = (float)(b.i / w) * keep * scale;
        maxvals[blockIdx.x] = b.v;
        if (idx) idx[blockIdx.x] = b.i;
    }
}

extern "C" int lh_heatmap_flip_merge(const float* a, const float* m, int bj, int h, int w, int shift, float scale, float* merged,
                                     float* preds, float* maxvals, int* idx, void* stream) {
    LH_REQUIRE(a && m && merged && preds && maxvals && bj > 0 && h > 0 && w > 0 && (long)h * w < (1L << 31),
               "lh_heatmap_flip_merge: bad arguments");
    const size_t bytes = (size_t)bj * h * w * sizeof(float);
    const auto apart = [bytes](const void* p, const void* q) {
        return (const char*)p + bytes <= (const char*)q || (const char*)q + bytes <= (const char*)p;
    };
    LH_REQUIRE(apart(m, merged) && (a == merged || apart(a, merged)),
               "lh_heatmap_flip_merge: merged may alias a exactly and must not overlap m");
    hipLaunchKernelGGL((heatmap_flip_merge_kernel<4>), dim3(bj), dim3(256), 0, (hipStream_t)stream, a, m, h * w, w, shift ? 1 : 0,
                       scale, merged, preds, maxvals, idx);
    LH_LAUNCH_CHECK("heatmap_flip_merge launch");
    return LH_OK;
}

// Opt-in soft-arg-max decode (named in the project's north star; NOT in the reference, which decodes with the hard arg-max
// of get_max_preds): preds = sum_p softmax(beta * hm)[p] * (x_p, y_p), computed per map with the usual max subtraction,
// fp32 exponentials and fp64 sums.  One workgroup per (sample, joint).
__global__ __launch_bounds__(256) void heatmap_soft_argmax_kernel(const float* hm, int hw, int w, float beta, float scale, float* preds) {
    __shared__ float rmax[4];
    __shared__ double rs[4][3];
    const float* m = hm + (long)blockIdx.x * hw;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < hw; i += 256) mx = fmaxf(mx, m[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) rmax[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
    double s0 = 0.0, sx = 0.0, sy = 0.0;
    for (int i = threadIdx.x; i < hw; i += 256) {
        const double e = (double)expf(beta * (m[i] - mx));
        s0 += e; sx += e * (double)(i % w); sy += e * (double)(i / w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o); }
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6][0] = s0; rs[threadIdx.x >> 6][1] = sx; rs[threadIdx.x >> 6][2] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t0 = rs[0][0] + rs[1][0] + rs[2][0] + rs[3][0];
        const double tx = rs[0][1] + rs[1][1] + rs[2][1] + rs[3][1];
        const double ty = rs[0][2] + rs[1][2] + rs[2][2] + rs[3][2];
        preds[blockIdx.x * 2 + 0] = (float)(tx / t0) * scale;
        preds[blockIdx.x * 2 + 1] = (float)(ty / t0) * scale;
    }
}

extern "C" int lh_heatmap_soft_argmax(const float* heatmaps, int bj, int h, int w, float beta, float scale, float* preds,
                                      void* stream) {
    LH_REQUIRE(heatmaps && preds && bj > 0 && h > 0 && w > 0, "lh_heatmap_soft_argmax: bad arguments");
    hipLaunchKernelGGL(heatmap_soft_argmax_kernel, dim3(bj), dim3(256), 0, (hipStream_t)stream, heatmaps, h * w, w, beta, scale, preds);
    LH_LAUNCH_CHECK("heatmap_soft_argmax launch");
    return LH_OK;
}

// ---- Integral-regression coordinate loss (Sun et al. 2018, "Integral Human Pose Regression"; an opt-in extension without a
// reference oracle): L1 between the soft-arg-max of a plane and its ground-truth joint, and the gradient of that through the
// softmax, added to the heat-map loss's outputs (lh_integral_l1).  One workgroup per plane:
//   1. the plane goes to LDS (h*w floats, sized by the launch: 16 KB for a 64 x 64 plane) with 16-byte loads, the maximum is
//      taken on the way;
//   2. e_p = expf(beta * (hm_p - max)) replaces the plane in LDS; S0, sum e x, sum e y in fp64 with the thread stride, the wave
//      shuffles and the four LDS slots of heatmap_soft_argmax_kernel, so preds has that kernel's bits;
//   3. every thread forms the expectation, the residual's signs and k_n from the slots, thread 0 stores preds and the plane's
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
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) rmax[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
    double s0 = 0.0, sx = 0.0, sy = 0.0;
    for (int i = tid; i < hw; i += 256) {                  // element i is read and replaced by this thread only
        const float ef = expf(beta * (plane[i] - mx));
        plane[i] = ef;
        const double e = (double)ef;
        s0 += e; sx += e * (double)(i % w); sy += e * (double)(i / w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o); }
    if ((tid & 63) == 0) { rs[tid >> 6][0] = s0; rs[tid >> 6][1] = sx; rs[tid >> 6][2] = sy; }
    __syncthreads();
    const double t0 = rs[0][0] + rs[1][0] + rs[2][0] + rs[3][0];
    const double ex = (rs[0][1] + rs[1][1] + rs[2][1] + rs[3][1]) / t0;
    const double ey = (rs[0][2] + rs[1][2] + rs[2][2] + rs[3][2]) / t0;
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

// ------------------------------------------------------------------------------------------------ validation metrics
// PCK_2d_loss(T, 'proportion') + EPE_train on the device (src/utils/loss.py:50-67,116-148): one wave per
// sample.  wrong[b] = #joints whose error / bbox-diagonal(gt) > T; epe[b] = sum of errors of joints 1..J-2 (the
// reference's joint range quirk).  Sums over the batch are left to the caller (device tensors, no host sync).
__global__ __launch_bounds__(64) void keypoint_metrics_kernel(const float* pred, const float* gt, int gt_stride, int j, float T,
                                                              int* wrong, float* epe) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* g = gt + (long)b * j * gt_stride;
    const float* p = pred + (long)b * j * 2;
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int k = lane; k < j; k += 64) {
        const float x = g[k * gt_stride], y = g[k * gt_stride + 1];
        xmin = fminf(xmin, x); xmax = fmaxf(xmax, x); ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        xmin = fminf(xmin, __shfl_xor(xmin, o)); xmax = fmaxf(xmax, __shfl_xor(xmax, o));
        ymin = fminf(ymin, __shfl_xor(ymin, o)); ymax = fmaxf(ymax, __shfl_xor(ymax, o));
    }
    const float diag = sqrtf((xmax - xmin) * (xmax - xmin) + (ymax - ymin) * (ymax - ymin));
    int w = 0;
    float e = 0.f;
    for (int k = lane; k < j; k += 64) {
        const float dx = g[k * gt_stride] - p[k * 2], dy = g[k * gt_stride + 1] - p[k * 2 + 1];
        const float dist = sqrtf(dx * dx + dy * dy);
        if (dist / diag > T) ++w;
        if (k >= 1 && k <= j - 2) e += dist;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { w += __shfl_xor(w, o); e += __shfl_xor(e, o); }
    if (lane == 0) { wrong[b] = w; epe[b] = e; }
}

extern "C" int lh_keypoint_metrics(const float* pred, const float* gt, int gt_stride, int b, int j, float T, int* wrong,
                                   float* epe, void* stream) {
    LH_REQUIRE(pred && gt && wrong && epe && b > 0 && j > 2 && gt_stride >= 2, "lh_keypoint_metrics: bad arguments");
    hipLaunchKernelGGL(keypoint_metrics_kernel, dim3(b), dim3(64), 0, (hipStream_t)stream, pred, gt, gt_stride, j, T, wrong, epe);
    LH_LAUNCH_CHECK("keypoint_metrics launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ PCK curve / AUC
// pred_eval (src/utils/argparser.py:326-388) on the device: for every threshold, the number of VISIBLE
// joints (gt[..][2] == 1) whose error -- pixel distance, divided by the sample's bbox size when bb is given ('pckb') --
// is < thr[t].  float64 like the NumPy original, integer atomics (exact, order independent: ranks add their counts with one
// small all-reduce).  diff_row[s] = sum of the pixel errors of ALL joints of sample s (the EPE numerator).
__global__ void pck_curve_kernel(const float* pred, const float* gt, int gt_stride, const float* bb, int n, int j,
                                 const double* thr, int nthr, unsigned long long* counts, unsigned long long* nvis,
                                 double* diff_row) {
    const int sidx = blockIdx.x;
    if (sidx >= n) return;
    __shared__ double err[64];
    __shared__ int vis[64];
    for (int k = threadIdx.x; k < j; k += blockDim.x) {
        const float* g = gt + ((long)sidx * j + k) * gt_stride;
        const float* q = pred + ((long)sidx * j + k) * 2;
        const double dx = (double)g[0] - (double)q[0], dy = (double)g[1] - (double)q[1];
        err[k] = sqrt(dx * dx + dy * dy);
        vis[k] = g[2] == 1.f ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        int nv = 0;
        for (int k = 0; k < j; ++k) { sum += err[k]; nv += vis[k]; }
        diff_row[sidx] = sum;
        if (nv) atomicAdd(nvis, (unsigned long long)nv);
    }
    const double scale = bb ? (double)bb[sidx] : 1.0;
    for (int t = threadIdx.x; t < nthr; t += blockDim.x) {
        int c = 0;
        for (int k = 0; k < j; ++k)
            if (vis[k] && err[k] / scale < thr[t]) ++c;
        if (c) atomicAdd(counts + t, (unsigned long long)c);
    }
}

extern "C" int lh_pck_curve(const float* pred, const float* gt, int gt_stride, const float* bb, int n, int j, const double* thr,
                            int nthr, unsigned long long* counts, unsigned long long* nvis, double* diff_row, void* stream) {
    LH_REQUIRE(pred && gt && thr && counts && nvis && diff_row && n > 0 && j > 0 && j <= 64 && gt_stride >= 3 && nthr > 0,
               "lh_pck_curve: bad arguments (j <= 64, gt rows of >= 3 values: x, y, visibility)");
    hipLaunchKernelGGL(pck_curve_kernel, dim3(n), dim3(128), 0, (hipStream_t)stream, pred, gt, gt_stride, bb, n, j, thr, nthr,
                       counts, nvis, diff_row);
    LH_LAUNCH_CHECK("pck_curve launch");
    return LH_OK;
}
