// Fused Adam (tick / apply / step) and dynamic loss scaling (inf / NaN check, scale update, guarded Adam).
#include "common.h"

// ------------------------------------------------------------------------------------------------ Adam
__device__ __forceinline__ void adam_tick(const double* hyper, int* step, float* derived) {
    const int t = *step + 1;
    *step = t;
    const double lr = hyper[0], b1 = hyper[1], b2 = hyper[2];
    derived[0] = (float)(lr / (1.0 - pow(b1, (double)t)));      // step size
    derived[1] = (float)sqrt(1.0 - pow(b2, (double)t));         // sqrt of bias correction 2
    derived[2] = (float)b1;
    derived[3] = (float)b2;
    derived[4] = (float)hyper[3];
}

__global__ void adam_tick_kernel(const double* hyper, int* step, float* derived) { adam_tick(hyper, step, derived); }

__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, long numel,
                                                   const float* derived, float gscale) {
    const float step_size = derived[0], bc2 = derived[1], b1 = derived[2], b2 = derived[3], eps = derived[4];
    const long nvec = numel / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float* P = &pp.x; const float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gk = G[k] * gscale;
            M[k] = M[k] * b1 + gk * (1.f - b1);
            V[k] = V[k] * b2 + gk * gk * (1.f - b2);
            P[k] -= step_size * (M[k] / (sqrtf(V[k]) / bc2 + eps));
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < numel; i += 256) {
            const float gk = g[i] * gscale;
            m[i] = m[i] * b1 + gk * (1.f - b1);
            v[i] = v[i] * b2 + gk * gk * (1.f - b2);
            p[i] -= step_size * (m[i] / (sqrtf(v[i]) / bc2 + eps));
        }
}

// Dynamic loss scaling (lh_adam_apply_guarded): adam_kernel's arithmetic with the gradient factor read from the device (*inv,
// written by amp_update_kernel), skipped whole when the step's gradients held an inf / NaN.  A kernel of its own rather than a
// flag of adam_kernel: routing adam_kernel through a shared inlined body, or making it a template, changes its code object
// (register assignment and schedule, kernel-argument layout, symbol), and the static path's kernel is kept as it was.
__global__ __launch_bounds__(256) void adam_kernel_guarded(float* p, const float* g, float* m, float* v, long numel,
                                                           const float* derived, const int* found_inf, const float* inv) {
    if (*found_inf) return;
    const float gscale = *inv;
    const float step_size = derived[0], bc2 = derived[1], b1 = derived[2], b2 = derived[3], eps = derived[4];
    const long nvec = numel / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float* P = &pp.x; const float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gk = G[k] * gscale;
            M[k] = M[k] * b1 + gk * (1.f - b1);
            V[k] = V[k] * b2 + gk * gk * (1.f - b2);
            P[k] -= step_size * (M[k] / (sqrtf(V[k]) / bc2 + eps));
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0)
        for (long i = nvec * 4 + threadIdx.x; i < numel; i += 256) {
            const float gk = g[i] * gscale;
            m[i] = m[i] * b1 + gk * (1.f - b1);
            v[i] = v[i] * b2 + gk * gk * (1.f - b2);
            p[i] -= step_size * (m[i] / (sqrtf(v[i]) / bc2 + eps));
        }
}

static int adam_grid(long numel) {
    const long nvec = numel / 4;
    return (int)((nvec + 255) / 256 > 2048 ? 2048 : ((nvec + 255) / 256 < 1 ? 1 : (nvec + 255) / 256));
}

extern "C" int lh_adam_tick(const double* hyper, int* step, float* derived, void* stream) {
    LH_REQUIRE(hyper && step && derived, "lh_adam_tick: null pointer");
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, hyper, step, derived);
    LH_LAUNCH_CHECK("adam_tick launch");
    return LH_OK;
}

extern "C" int lh_adam_apply(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long numel, const float* derived,
                             float grad_scale, void* stream) {
    LH_REQUIRE(param && grad && exp_avg && exp_avg_sq && derived && numel > 0, "lh_adam_apply: bad arguments");
    LH_REQUIRE((((size_t)param | (size_t)grad | (size_t)exp_avg | (size_t)exp_avg_sq) & 15) == 0, "lh_adam_apply: slices must start on 16-byte boundaries");
    hipLaunchKernelGGL(adam_kernel, dim3(adam_grid(numel)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, numel,
                       derived, grad_scale);
    LH_LAUNCH_CHECK("adam launch");
    return LH_OK;
}

extern "C" int lh_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long numel,
                            const double* hyper, int* step, float* derived, float grad_scale, void* stream) {
    LH_REQUIRE(param && grad && exp_avg && exp_avg_sq && hyper && step && derived && numel > 0, "lh_adam_step: bad arguments");
    const int rc = lh_adam_tick(hyper, step, derived, stream);
    if (rc) return rc;
    return lh_adam_apply(param, grad, exp_avg, exp_avg_sq, numel, derived, grad_scale, stream);
}

// ------------------------------------------------------------------------------------------------ dynamic loss scaling
// torch.amp.GradScaler + optimizer.step() as three launches inside the captured step, no host decision:
//   amp_check_kernel     every workgroup ORs "some element is inf / NaN" over its share of the RAW gradient arena (before
//                        unscaling, as torch._amp_foreach_non_finite_check_and_unscale_) into ITS slot of `partial`: every slot
//                        is overwritten at every replay, so neither atomics nor a memset node are needed;
//   amp_update_kernel    one workgroup: found_inf = OR of the slots, inv = extra / scale, the scale update of
//                        torch._amp_update_scale_, skipped += found_inf, and -- only for a finite step -- the Adam tick;
//   adam_kernel_guarded  the Adam update with gscale = *inv, skipped whole when *found_inf.
// The next kernel on the stream reads what the previous one stored: kernel boundaries order the hand-offs.
constexpr int AMP_CHECK_BLOCKS = 2048;      // 8 workgroups of 4 waves per CU: ~32 KiB of loads in flight per CU, HBM rate

__device__ __forceinline__ bool lh_not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
// 0 when the exponent field is all ones (inf / NaN): four elements tested with one compare, no branch
__device__ __forceinline__ unsigned lh_exp_gap(float x) { return (__float_as_uint(x) & 0x7f800000u) ^ 0x7f800000u; }

__global__ __launch_bounds__(256) void amp_check_kernel(const float* g, long numel, int* partial) {
    __shared__ int red[4];
    const long nvec = numel / 4;
    bool bad = false;           // wave-uniform: one __any per iteration
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const float4 v = lh_ld_nt(reinterpret_cast<const float4*>(g) + i);   // the gradient's last read before Adam's
        bad |= __any(min(min(lh_exp_gap(v.x), lh_exp_gap(v.y)), min(lh_exp_gap(v.z), lh_exp_gap(v.w))) == 0u);
    }
    if (blockIdx.x == 0 && nvec * 4 + threadIdx.x < numel) bad |= lh_not_finite(g[nvec * 4 + threadIdx.x]);
    bad = __any(bad);           // lanes leave the loop one iteration apart
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] | red[1] | red[2] | red[3];
}

// amp_hyper = {growth_factor, backoff_factor, growth_interval} (fp64 on the device: a loaded state dict takes effect without
// a recapture).  Arithmetic of torch._amp_update_scale_: the factor products are formed in fp64 and rounded to fp32 once.
__global__ __launch_bounds__(256) void amp_update_kernel(const int* partial, int npartial, const double* amp_hyper, float* scale,
                                                         int* growth_tracker, int* found_inf, int* skipped, float* inv, double extra,
                                                         const double* hyper, int* step, float* derived) {
    __shared__ int red[4];
    int bad = 0;
    for (int i = threadIdx.x; i < npartial; i += 256) bad |= partial[i];
    bad = __any(bad != 0);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int inf = red[0] | red[1] | red[2] | red[3];
    const float s = *scale;
    *found_inf = inf;
    *inv = (float)(extra / (double)s);        // GradScaler: scale.double().reciprocal().float(); the static path: host fp64
    *skipped += inf;
    if (inf) {
        *scale = (float)((double)s * amp_hyper[1]);
        *growth_tracker = 0;
        return;                                // Adam's step counter and derived values stay as they are
    }
    const int successful = *growth_tracker + 1;
    if ((double)successful == amp_hyper[2]) {
        const float grown = (float)((double)s * amp_hyper[0]);
        if (!lh_not_finite(grown)) *scale = grown;
        *growth_tracker = 0;
    } else {
        *growth_tracker = successful;
    }
    adam_tick(hyper, step, derived);
}

extern "C" int lh_amp_check_blocks(void) { return AMP_CHECK_BLOCKS; }

extern "C" int lh_amp_check(const float* grad, long numel, int* partial, void* stream) {
    LH_REQUIRE(grad && partial && numel > 0, "lh_amp_check: bad arguments");
    LH_REQUIRE(((size_t)grad & 15) == 0, "lh_amp_check: the gradient must start on a 16-byte boundary");
    hipLaunchKernelGGL(amp_check_kernel, dim3(AMP_CHECK_BLOCKS), dim3(256), 0, (hipStream_t)stream, grad, numel, partial);
    LH_LAUNCH_CHECK("amp_check launch");
    return LH_OK;
}

extern "C" int lh_amp_update(const int* partial, const double* amp_hyper, float* scale, int* growth_tracker, int* found_inf,
                             int* skipped, float* inv, double extra, const double* hyper, int* step, float* derived, void* stream) {
    LH_REQUIRE(partial && amp_hyper && scale && growth_tracker && found_inf && skipped && inv && hyper && step && derived,
               "lh_amp_update: null pointer");
    hipLaunchKernelGGL(amp_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, AMP_CHECK_BLOCKS, amp_hyper, scale,
                       growth_tracker, found_inf, skipped, inv, extra, hyper, step, derived);
    LH_LAUNCH_CHECK("amp_update launch");
    return LH_OK;
}

extern "C" int lh_adam_apply_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long numel,
                                     const float* derived, const int* found_inf, const float* inv, void* stream) {
    LH_REQUIRE(param && grad && exp_avg && exp_avg_sq && derived && found_inf && inv && numel > 0, "lh_adam_apply_guarded: bad arguments");
    LH_REQUIRE((((size_t)param | (size_t)grad | (size_t)exp_avg | (size_t)exp_avg_sq) & 15) == 0,
               "lh_adam_apply_guarded: buffers must start on 16-byte boundaries");
    hipLaunchKernelGGL(adam_kernel_guarded, dim3(adam_grid(numel)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                       numel, derived, found_inf, inv);
    LH_LAUNCH_CHECK("adam_guarded launch");
    return LH_OK;
}
