// BatchNorm statistics of a dense activation, the fold + finalize of a statistics slab (one layer, or several as one
// launch) and the eval-mode affine.
#include "bn_common.h"
#include "multi.h"

// Column sums of a [rows][ncol] slab in double: block = 16 columns x 16 row lanes.
template <typename TI>
__global__ __launch_bounds__(256) void colsum_kernel(const TI* src, int rows, int ncol, int rows_per_block,
                                                     double* dst) {
    __shared__ double red[16][17];
    const int col = blockIdx.x * 16 + (threadIdx.x & 15), rl = threadIdx.x >> 4;
    const int r0 = blockIdx.y * rows_per_block;
    int r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    double a = 0.0;
    if (col < ncol)
        for (int r = r0 + rl; r < r1; r += 16) a += (double)src[(long)r * ncol + col];
    red[rl][threadIdx.x & 15] = a;
    __syncthreads();
    if (threadIdx.x < 16) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += red[i][threadIdx.x];
        if (col < ncol) dst[(long)blockIdx.y * ncol + col] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// Generic stats of a dense [m][c] activation (the conv kernels normally produce these slabs
// in their epilogue; this kernel serves tensors that did not come out of lh_igemm).
constexpr int STAT_ROWS = 128;

template <typename T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T* y, int m, int c, float* stats) {
    constexpr int EPC = 16 / sizeof(T);
    const int nchunk = c / EPC;
    const long r0 = (long)blockIdx.x * STAT_ROWS;
    float* out = stats + (long)blockIdx.x * 2 * c;
    for (int ch = threadIdx.x; ch < nchunk; ch += 256) {
        float s1[EPC], s2[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) s1[e] = s2[e] = 0.f;
        for (int r = 0; r < STAT_ROWS && r0 + r < m; ++r) {
            float v[EPC];
            unpack16<T>(*reinterpret_cast<const uint4*>(y + (r0 + r) * c + ch * EPC), v);
#pragma unroll
            for (int e = 0; e < EPC; ++e) { s1[e] += v[e]; s2[e] += v[e] * v[e]; }
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) { out[ch * EPC + e] = s1[e]; out[c + ch * EPC + e] = s2[e]; }
    }
}

extern "C" int lh_bn_stats_rows(int m, int c) { (void)c; return ceil_div(m, STAT_ROWS); }

extern "C" int lh_bn_stats(const void* y, int m, int c, float* stats, int* rows_out, int dtype, void* stream) {
    LH_REQUIRE(y && stats && m > 0 && c > 0, "lh_bn_stats: bad arguments");
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0 && c % (16 / es) == 0, "lh_bn_stats: c %d not a multiple of %d", c, 16 / (es > 0 ? es : 1));
    const int rows = ceil_div(m, STAT_ROWS);
    if (rows_out) *rows_out = rows;
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((bn_stats_kernel<T>), dim3(rows), dim3(256), 0, (hipStream_t)stream,
                                                   (const T*)y, m, c, stats));
    LH_LAUNCH_CHECK("bn_stats launch");
    return LH_OK;
}

extern "C" size_t lh_bn_stats_slab_bytes(int rows, int c) {
    return ((size_t)rows * 2 * c + 2) * 4 + (size_t)(ceil_div(rows, 256) + 1) * 2 * c * 8;
}

template <typename TI> struct bn_finalize_fused {
using Args = FinalizeArgs;
static __device__ __forceinline__ void run(const FinalizeArgs& p, const int bid, const int nblk) {
    if (bid == 0 && threadIdx.x == 0 && p.nbt) *p.nbt += 1;
    auto fin = [&](int ch, double s0, double s1) { float sc, sh; bn_finalize_channel(p, ch, s0, s1, true, sc, sh); };
    if (p.rows >= LH_FOLD_WIDE_ROWS) slab_totals_then64((const TI*)p.slab, p.rows, p.c, bid, fin);
    else slab_totals_then((const TI*)p.slab, p.rows, p.c, bid, fin);
}
};

// stats: [rows][2][c] floats followed by scratch for (ceil(rows/256) + 1) * 2c doubles.
static FinalizeArgs finalize_args(const void* slab, int rows, int count, int c, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, long long* nbt, float momentum, float eps, float* scale, float* shift,
                                  float* save_mean, float* save_invstd) {
    FinalizeArgs a;
    a.slab = slab; a.rows = rows; a.count = count; a.c = c; a.gamma = gamma; a.beta = beta; a.rmean = running_mean; a.rvar = running_var;
    a.nbt = nbt; a.momentum = momentum; a.eps = eps; a.scale = scale; a.shift = shift; a.smean = save_mean; a.sinv = save_invstd;
    return a;
}

extern "C" int lh_bn_finalize(const float* stats, int rows, int count, int c, const float* gamma,
                              const float* beta, float* running_mean, float* running_var,
                              long long* num_batches_tracked, float momentum, float eps, float* scale,
                              float* shift, float* save_mean, float* save_invstd, void* stream) {
    LH_REQUIRE(stats && scale && shift && rows > 0 && count > 0 && c > 0, "lh_bn_finalize: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const long slab_floats = (long)rows * 2 * c;
    double* scratch = (double*)(stats + ((slab_floats + 1) & ~1L));
    if (rows <= 1024) {      // one launch: fold the slab and finalize
        const FinalizeArgs a = finalize_args(stats, rows, count, c, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                                             scale, shift, save_mean, save_invstd);
        hipLaunchKernelGGL((lh_one_kernel<bn_finalize_fused<float>>), dim3(fold_grid(rows, c)), dim3(256), 0, s, a);
        LH_LAUNCH_CHECK("bn_finalize launch");
        return LH_OK;
    }
    // two launches: 256-row partial folds (fp64), then fold + finalize
    const int gy = ceil_div(rows, 256);
    hipLaunchKernelGGL((colsum_kernel<float>), dim3(ceil_div(2 * c, 16), gy), dim3(256), 0, s, stats, rows, 2 * c, 256, scratch);
    const FinalizeArgs a = finalize_args(scratch, gy, count, c, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                                         scale, shift, save_mean, save_invstd);
    hipLaunchKernelGGL((lh_one_kernel<bn_finalize_fused<double>>), dim3(fold_grid(gy, c)), dim3(256), 0, s, a);
    LH_LAUNCH_CHECK("bn_finalize launch");
    return LH_OK;
}

// The same folds for up to n independent BatchNorm layers as ONE launch (multi.h); layers whose slab has more than 1024
// rows take the two-launch path of lh_bn_finalize one by one.
extern "C" int lh_bn_finalize_multi(const lh_bn_finalize_call* calls, int n, void* stream) {
    LH_REQUIRE(calls && n >= 1, "lh_bn_finalize_multi: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    FinalizeArgs a[LH_MULTI_MAX];
    const FinalizeArgs* ap[LH_MULTI_MAX];
    int grid[LH_MULTI_MAX], m = 0;
    for (int i = 0; i < LH_MULTI_MAX; ++i) ap[i] = &a[i];
    auto flush = [&]() -> int {
        if (m == 0) return LH_OK;
        lh_launch<bn_finalize_fused<float>>(ap, grid, m, s);
        LH_LAUNCH_CHECK("bn_finalize_multi launch");
        m = 0;
        return LH_OK;
    };
    for (int i = 0; i < n; ++i) {
        const lh_bn_finalize_call& q = calls[i];
        LH_REQUIRE(q.stats && q.scale && q.shift && q.rows > 0 && q.count > 0 && q.c > 0, "lh_bn_finalize_multi: bad arguments (layer %d)", i);
        if (q.rows > 1024) {
            const int rc = lh_bn_finalize(q.stats, q.rows, q.count, q.c, q.gamma, q.beta, q.running_mean, q.running_var, q.num_batches_tracked,
                                          q.momentum, q.eps, q.scale, q.shift, q.save_mean, q.save_invstd, stream);
            if (rc) return rc;
            continue;
        }
        a[m] = finalize_args(q.stats, q.rows, q.count, q.c, q.gamma, q.beta, q.running_mean, q.running_var, q.num_batches_tracked,
                             q.momentum, q.eps, q.scale, q.shift, q.save_mean, q.save_invstd);
        grid[m] = fold_grid(q.rows, q.c);
        if (++m == LH_MULTI_MAX) { const int rc = flush(); if (rc) return rc; }
    }
    return flush();
}

__global__ void bn_eval_affine_kernel(const float* gamma, const float* beta, const float* rm, const float* rv,
                                      float eps, int c, float* scale, float* shift) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    const float sc = gamma[ch] / sqrtf(rv[ch] + eps);
    scale[ch] = sc;
    shift[ch] = beta[ch] - rm[ch] * sc;
}

extern "C" int lh_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, float eps, int c, float* scale, float* shift,
                                 void* stream) {
    LH_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && c > 0, "lh_bn_eval_affine: bad arguments");
    hipLaunchKernelGGL(bn_eval_affine_kernel, dim3(ceil_div(c, 128)), dim3(128), 0, (hipStream_t)stream, gamma, beta,
                       running_mean, running_var, eps, c, scale, shift);
    LH_LAUNCH_CHECK("bn_eval_affine launch");
    return LH_OK;
}
