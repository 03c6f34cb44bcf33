// The fused "sum of affine terms (+ nearest upsample) + ReLU" elementwise op, backward: per BatchNorm term a reduce pass
// (partial sums of g and g * xhat), a coefficient fold and an apply pass; one node, or several independent nodes phase by phase.
#include "bn_common.h"
#include "multi.h"
#include <type_traits>
#include <vector>
#include <algorithm>

// ------------------------------------------------------------------------------------------------
// Backward of one term.  g = dout * (out > 0) summed over the term's 2^l x 2^l upsampling cell.
struct FuseBwdArgs {
    const unsigned char* dout;
    const unsigned char* out;
    const unsigned char* mask;   // optional ReLU mask bits written by lh_fuse_fwd (replaces reading `out`)
    const unsigned char* x;      // raw BN input of this term (null: identity)
    const float* scale;
    const float* mean;
    const float* invstd;
    unsigned char* dx;
    float* partial;              // [strips][2][c]
    const double* totals;        // [2][c]
    float* coef;                 // [2][c]: mean(g), mean(g*xhat)
    float* dgamma;
    float* dbeta;
    int n, h, w, c;              // OUTPUT resolution
    int l, relu, accumulate;
    int mask_from_x;             // ReLU mask recomputed from x*scale+shift (single BN term): `out` is not read
    const float* shift;
    int rows_per_strip;
    const unsigned char* touch;  // optional (lh_fuse_bwd_desc.l2_touch): the last apply launch of the call warms it in L2 (lh_l2_touch)
    unsigned touch_bytes;
    long count;                  // n * (h>>l) * (w>>l)
    long total;                  // 16-byte chunks of dx (flat apply kernel)
    int fold_rows;               // > 0: the flat apply pass folds partial[fold_rows][2][c] itself (no coefficient launch)
    int exp;                     // bn_exp_flags() & 3 (backward bits)
};

// Two terms, no upsampling (the residual-unit tail: BN(main) + identity | BN(shortcut)): ONE pass reads dout / out once
// and writes both input gradients.  Term k: BN when x[k] != null (dx = A*g + B*x + C) else identity (dx = g).
struct FuseBwd2Args {
    const unsigned char* dout;
    const unsigned char* out;
    const unsigned char* mask;
    const unsigned char* x[2];
    const float* scale[2];
    const float* mean[2];
    const float* invstd[2];
    const float* coef[2];
    unsigned char* dx[2];
    int accumulate[2];
    int c, relu;
    long total;
    const float* fold_slab[2];   // term k folds fold_slab[k][fold_rows[k]][2][c] itself (see fold_coef_block); null: coef[k]
    int fold_rows[2];
    const unsigned char* touch;  // optional: lh_l2_touch at the tail
    unsigned touch_bytes;
    long count;
    float* dgamma[2];
    float* dbeta[2];
    int exp;                     // bn_exp_flags() & 3
};

struct CoefArgs {
    const float* slab;           // [rows][2][c]
    int rows, c;
    long count;
    float* coef;
    float* dgamma;
    float* dbeta;
};

// the passes (a launch record's kind; the mixed kernels take it as a per-problem tag)
enum BwdKind { K_FB_REDUCE_GEN, K_FB_REDUCE_FLAT, K_FB_REDUCE_FLAT_X, K_FB_COEF, K_FB_APPLY_GEN, K_FB_APPLY_FLAT, K_FB_APPLY_FLAT_X,
               K_FB_APPLY2 };

template <typename T, int EPC>
__device__ __forceinline__ void cell_grad(const FuseBwdArgs& p, int n, int ys, int xs, int chunk, float* g) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) g[e] = 0.f;
    const int f = 1 << p.l;
    for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) {
            const long pix = ((long)n * p.h + (ys << p.l) + dy) * p.w + (xs << p.l) + dx;
            const long off = (pix * p.c + chunk * EPC) * sizeof(T);
            float d[EPC];
            unpack16<T>(*reinterpret_cast<const uint4*>(p.dout + off), d);
            if (p.relu && p.mask) {
                mask_by_bits<EPC>(p.mask[off >> 4], d);
            } else if (p.relu) {
                float o[EPC];
                unpack16<T>(*reinterpret_cast<const uint4*>(p.out + off), o);
#pragma unroll
                for (int e = 0; e < EPC; ++e) d[e] = o[e] > 0.f ? d[e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] += d[e];
        }
}

template <typename T> struct fuse_bwd_reduce {
using Args = FuseBwdArgs;
static __device__ __forceinline__ void run(const FuseBwdArgs& p, const int bid, const int nblk) {
    constexpr int EPC = 16 / sizeof(T);
    __shared__ float red[256 * EPC * 2];
    const int nchunk = p.c / EPC;
    const int hs = p.h >> p.l, ws = p.w >> p.l;
    const long r0 = (long)bid * p.rows_per_strip;
    long r1 = r0 + p.rows_per_strip;
    if (r1 > p.count) r1 = p.count;
    float* out = p.partial + (long)bid * 2 * p.c;
    // active threads: a whole number of row lanes over the chunks (chunk fixed per thread)
    for (int cb = 0; cb < nchunk; cb += 256) {
        const int nc = nchunk - cb < 256 ? nchunk - cb : 256;
        const int lanes = 256 / nc;
        const int chunk = cb + (int)(threadIdx.x % nc), rl = threadIdx.x / nc;
        float s1[EPC], s2[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) s1[e] = s2[e] = 0.f;
        if (rl < lanes) {
            float mean[EPC], inv[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) { mean[e] = p.mean[chunk * EPC + e]; inv[e] = p.invstd[chunk * EPC + e]; }
            for (long r = r0 + rl; r < r1; r += lanes) {
                const unsigned t2 = (unsigned)r / (unsigned)ws;          // 32-bit: count < 2^31 (plan_fuse_bwd)
                const int xs = (int)((unsigned)r - t2 * (unsigned)ws);
                const int n = (int)(t2 / (unsigned)hs), ys = (int)(t2 - (unsigned)n * (unsigned)hs);
                float g[EPC], xv[EPC];
                cell_grad<T, EPC>(p, n, ys, xs, chunk, g);
                unpack16<T>(*reinterpret_cast<const uint4*>(p.x + (r * p.c + chunk * EPC) * sizeof(T)), xv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) { s1[e] += g[e]; s2[e] += g[e] * (xv[e] - mean[e]) * inv[e]; }
            }
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) { red[(threadIdx.x * EPC + e) * 2] = s1[e]; red[(threadIdx.x * EPC + e) * 2 + 1] = s2[e]; }
        __syncthreads();
        for (int t = threadIdx.x; t < nc * EPC; t += 256) {
            const int cl = t / EPC, e = t % EPC;
            float a = 0.f, b = 0.f;
            for (int k = 0; k < lanes; ++k) { a += red[((k * nc + cl) * EPC + e) * 2]; b += red[((k * nc + cl) * EPC + e) * 2 + 1]; }
            out[(cb + cl) * EPC + e] = a;
            out[p.c + (cb + cl) * EPC + e] = b;
        }
        __syncthreads();
    }
}
};

template <typename T> struct fuse_bwd_apply {
using Args = FuseBwdArgs;
static __device__ __forceinline__ void run(const FuseBwdArgs& p, const int bid, const int nblk) {
    constexpr int EPC = 16 / sizeof(T);
    const int nchunk = p.c / EPC;
    const int hs = p.h >> p.l, ws = p.w >> p.l;
    const long total = p.count * nchunk;
    for (long idx = (long)bid * 256 + threadIdx.x; idx < total; idx += (long)nblk * 256) {
        const unsigned iu = (unsigned)idx;                               // 32-bit: total < 2^31 (plan_fuse_bwd)
        const unsigned r = iu / (unsigned)nchunk;
        const int chunk = (int)(iu - r * (unsigned)nchunk);
        const unsigned t2 = r / (unsigned)ws;
        const int xs = (int)(r - t2 * (unsigned)ws);
        const int n = (int)(t2 / (unsigned)hs), ys = (int)(t2 - (unsigned)n * (unsigned)hs);
        float g[EPC];
        cell_grad<T, EPC>(p, n, ys, xs, chunk, g);
        if (p.x) {
            float xv[EPC];
            unpack16<T>(*reinterpret_cast<const uint4*>(p.x + idx * 16), xv);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const int ch = chunk * EPC + e;
                const float xh = (xv[e] - p.mean[ch]) * p.invstd[ch];
                g[e] = p.scale[ch] * (g[e] - p.coef[ch] - xh * p.coef[p.c + ch]);
            }
        }
        uint4* dst = reinterpret_cast<uint4*>(p.dx + idx * 16);
        if (p.accumulate) {
            float o[EPC];
            unpack16<T>(*dst, o);
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] += o[e];
        }
        *dst = pack16<T>(g);
    }
}
};

// Coefficient fold INSIDE the apply pass (small tensors only, plan_fuse_bwd): every workgroup folds the reduce pass's
// [rows][2][c] partial sums itself -- rows * 2c <= 16 Ki floats, all of its loads in flight at once, fp64 sums in a fixed
// order, so every workgroup gets bit-identical coefficients -- and the separate fold launch (5-6 us on the dependency chain
// of every BatchNorm of HRNet's branches) disappears.  coefL[0..c) = mean(g), coefL[c..2c) = mean(g * xhat); workgroup 0
// also stores the parameter gradients dbeta = sum(g), dgamma = sum(g * xhat).
constexpr int LH_FOLD_IN_APPLY_FLOATS = 16384;
__device__ __forceinline__ void fold_coef_block(const float* slab, int rows, int c, long count, float* dgamma, float* dbeta,
                                                bool writer, float* coefL) {
    __shared__ double fold_part[512];
    const int ncol = 2 * c;                              // power of two, <= 512
    const int t = threadIdx.x;
    if (ncol <= 256) {
        const int parts = 256 / ncol, col = t & (ncol - 1), part = t / ncol;
        double a = 0.0;
        int r = part;
        for (; r + 7 * parts < rows; r += 8 * parts) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = slab[(long)(r + u * parts) * ncol + col];
#pragma unroll
            for (int u = 0; u < 8; ++u) a += (double)v[u];
        }
        for (; r < rows; r += parts) a += (double)slab[(long)r * ncol + col];
        fold_part[t] = a;
        __syncthreads();
        if (t < ncol) {
            double tot = 0.0;
            for (int q = 0; q < parts; ++q) tot += fold_part[q * ncol + t];
            coefL[t] = (float)(tot / (double)count);
            if (writer) {
                if (t < c) { if (dbeta) dbeta[t] = (float)tot; }
                else if (dgamma) dgamma[t - c] = (float)tot;
            }
        }
    } else {                                             // 2c = 512: two columns per thread, every row
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int col = t + 256 * h;
            double a = 0.0;
            int r = 0;
            for (; r + 8 <= rows; r += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = slab[(long)(r + u) * ncol + col];
#pragma unroll
                for (int u = 0; u < 8; ++u) a += (double)v[u];
            }
            for (; r < rows; ++r) a += (double)slab[(long)r * ncol + col];
            coefL[col] = (float)(a / (double)count);
            if (writer) {
                if (col < c) { if (dbeta) dbeta[col] = (float)a; }
                else if (dgamma) dgamma[col - c] = (float)a;
            }
        }
    }
    __syncthreads();
}

// ---- l == 0 fast paths: dout / out / x / dx share one flat element offset, the thread keeps one channel chunk.
template <typename T, bool MASK_X> struct fuse_bwd_reduce_flat {
using Args = FuseBwdArgs;
static __device__ __forceinline__ void run(const FuseBwdArgs& p, const int bid, const int nblk) {
    constexpr int EPC = 16 / sizeof(T);
    __shared__ float red[256 * EPC * 2];
    const int nchunk = p.c / EPC;                       // power of two <= 256
    const int lanes = 256 / nchunk;
    const int chunk = threadIdx.x & (nchunk - 1), rl = threadIdx.x / nchunk;
    const long r0 = (long)bid * p.rows_per_strip;
    long r1 = r0 + p.rows_per_strip;
    if (r1 > p.count) r1 = p.count;
    float mean[EPC], inv[EPC], sc[EPC], sh[EPC], s1[EPC], s2[EPC];
    load_vec<EPC>(p.mean + chunk * EPC, mean);
    load_vec<EPC>(p.invstd + chunk * EPC, inv);
    if (MASK_X) { load_vec<EPC>(p.scale + chunk * EPC, sc); load_vec<EPC>(p.shift + chunk * EPC, sh); }
    fill_vec<EPC>(s1, 0.f);
    fill_vec<EPC>(s2, 0.f);
    const long rowb = (long)p.c * sizeof(T);
    // one row of this thread's channel chunk: gate the gradient, accumulate (rows in ascending order: the sums do not
    // depend on how many rows are fetched ahead)
    auto row = [&](const uint4& gd, const uint4& xd, unsigned mbits, const uint4& od) __attribute__((always_inline)) {
        float g[EPC], xv[EPC];
        unpack16<T>(gd, g);
        unpack16<T>(xd, xv);
        if (MASK_X) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] = (xv[e] * sc[e] + sh[e]) > 0.f ? g[e] : 0.f;
        } else if (p.relu && p.mask) {
            mask_by_bits<EPC>(mbits, g);
        } else if (p.relu) {
            float o[EPC];
            unpack16<T>(od, o);
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] = o[e] > 0.f ? g[e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) { s1[e] += g[e]; s2[e] += g[e] * (xv[e] - mean[e]) * inv[e]; }
    };
    const bool bits = !MASK_X && p.relu && p.mask, outs = !MASK_X && p.relu && !p.mask;
    constexpr int UN = MASK_X ? 1 : 4;      // rows fetched ahead per thread (measured: the mask-from-x form, with 16 more registers, is faster without)
    long r = r0 + rl;
    for (; r + (UN - 1) * (long)lanes < r1; r += UN * (long)lanes) {
        uint4 gd[UN], xd[UN], od[UN];
        unsigned mb[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const long off = (r + u * (long)lanes) * rowb + chunk * 16;
            gd[u] = *reinterpret_cast<const uint4*>(p.dout + off);
            xd[u] = *reinterpret_cast<const uint4*>(p.x + off);
            mb[u] = bits ? p.mask[off >> 4] : 0u;
            od[u] = outs ? *reinterpret_cast<const uint4*>(p.out + off) : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) row(gd[u], xd[u], mb[u], od[u]);
    }
    for (; r < r1; r += lanes) {
        const long off = r * rowb + chunk * 16;
        row(*reinterpret_cast<const uint4*>(p.dout + off), *reinterpret_cast<const uint4*>(p.x + off), bits ? p.mask[off >> 4] : 0u,
            outs ? *reinterpret_cast<const uint4*>(p.out + off) : uint4{0u, 0u, 0u, 0u});
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) { red[(threadIdx.x * EPC + e) * 2] = s1[e]; red[(threadIdx.x * EPC + e) * 2 + 1] = s2[e]; }
    __syncthreads();
    float* out = p.partial + (long)bid * 2 * p.c;
    for (int t = threadIdx.x; t < nchunk * EPC; t += 256) {
        const int cl = t / EPC, e = t % EPC;
        float a = 0.f, b = 0.f;
        for (int k = 0; k < lanes; ++k) { a += red[((k * nchunk + cl) * EPC + e) * 2]; b += red[((k * nchunk + cl) * EPC + e) * 2 + 1]; }
        out[cl * EPC + e] = a;
        out[p.c + cl * EPC + e] = b;
    }
}
};

template <typename T, bool MASK_X> struct fuse_bwd_apply_flat {
using Args = FuseBwdArgs;
static __device__ __forceinline__ void run(const FuseBwdArgs& p, const int bid, const int nblk) {
    const long total = p.total;
    constexpr int EPC = 16 / sizeof(T);
    const int nchunk = p.c / EPC;
    const int chunk = threadIdx.x & (nchunk - 1);
    // dx = scale*(g - c0 - xhat*c1) = A*g + B*x + C  with  xhat = (x - mean)*invstd
    float A[EPC], B[EPC], Cc[EPC], sc[EPC], sh[EPC];
    if (p.x) {
        float iv[EPC], c0[EPC], c1[EPC], mn[EPC];
        load_vec<EPC>(p.scale + chunk * EPC, A);
        load_vec<EPC>(p.invstd + chunk * EPC, iv);
        if (p.fold_rows > 0) {
            __shared__ float coefL[512];
            fold_coef_block(p.partial, p.fold_rows, p.c, p.count, p.dgamma, p.dbeta, bid == 0, coefL);
#pragma unroll
            for (int e = 0; e < EPC; ++e) { c0[e] = coefL[chunk * EPC + e]; c1[e] = coefL[p.c + chunk * EPC + e]; }
        } else {
            load_vec<EPC>(p.coef + chunk * EPC, c0);
            load_vec<EPC>(p.coef + p.c + chunk * EPC, c1);
        }
        load_vec<EPC>(p.mean + chunk * EPC, mn);
#pragma unroll
        for (int e = 0; e < EPC; ++e) { B[e] = -A[e] * iv[e] * c1[e]; Cc[e] = -A[e] * c0[e] - B[e] * mn[e]; }
        if (MASK_X) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) sc[e] = A[e];
            load_vec<EPC>(p.shift + chunk * EPC, sh);
        }
    } else { fill_vec<EPC>(A, 1.f); fill_vec<EPC>(B, 0.f); fill_vec<EPC>(Cc, 0.f); }
    const long stride = (long)nblk * 256;
    const long rounds = (total + stride - 1) / stride;
    const bool rev = p.exp & 2;
    auto body = [&](auto NTc) __attribute__((always_inline)) {
    constexpr bool LNT = decltype(NTc)::value;
    for (long rr = 0; rr < rounds; ++rr) {
        const long idx = walk_round(rr, rounds, rev) * stride + (long)bid * 256 + threadIdx.x;
        if (idx >= total) continue;
        const long off = idx * 16;
        float g[EPC], xv[EPC];
        unpack16<T>(ld16<LNT>(p.dout + off), g);
        if (p.x) unpack16<T>(ld16<LNT>(p.x + off), xv);
        if (MASK_X) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] = (xv[e] * sc[e] + sh[e]) > 0.f ? g[e] : 0.f;
        } else if (p.relu && p.mask) {
            mask_by_bits<EPC>(p.mask[off >> 4], g);
        } else if (p.relu) {
            float o[EPC];
            unpack16<T>(ld16<LNT>(p.out + off), o);
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] = o[e] > 0.f ? g[e] : 0.f;
        }
        if (p.x) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] = A[e] * g[e] + B[e] * xv[e] + Cc[e];
        }
        uint4* dst = reinterpret_cast<uint4*>(p.dx + off);
        if (p.accumulate) {
            float o[EPC];
            unpack16<T>(*dst, o);
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] += o[e];
        }
        *dst = pack16<T>(g);
    }
    };
    if (p.exp & 1) body(std::true_type{}); else body(std::false_type{});
    lh_l2_touch(p.touch, p.touch_bytes, bid, nblk);
}
};

template <typename T> struct fuse_bwd_apply2_flat {
using Args = FuseBwd2Args;
static __device__ __forceinline__ void run(const FuseBwd2Args& p, const int bid, const int nblk) {
    const long total = p.total;
    constexpr int EPC = 16 / sizeof(T);
    const int nchunk = p.c / EPC;
    const int chunk = threadIdx.x & (nchunk - 1);
    float A[2][EPC], B[2][EPC], Cc[2][EPC];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (p.x[k]) {
            float iv[EPC], c0[EPC], c1[EPC], mn[EPC];
            load_vec<EPC>(p.scale[k] + chunk * EPC, A[k]);
            load_vec<EPC>(p.invstd[k] + chunk * EPC, iv);
            if (p.fold_slab[k]) {
                __shared__ float coefL2[512];
                if (k) __syncthreads();                  // the other term's coefficients have been read by every thread
                fold_coef_block(p.fold_slab[k], p.fold_rows[k], p.c, p.count, p.dgamma[k], p.dbeta[k], bid == 0, coefL2);
#pragma unroll
                for (int e = 0; e < EPC; ++e) { c0[e] = coefL2[chunk * EPC + e]; c1[e] = coefL2[p.c + chunk * EPC + e]; }
            } else {
                load_vec<EPC>(p.coef[k] + chunk * EPC, c0);
                load_vec<EPC>(p.coef[k] + p.c + chunk * EPC, c1);
            }
            load_vec<EPC>(p.mean[k] + chunk * EPC, mn);
#pragma unroll
            for (int e = 0; e < EPC; ++e) { B[k][e] = -A[k][e] * iv[e] * c1[e]; Cc[k][e] = -A[k][e] * c0[e] - B[k][e] * mn[e]; }
        } else { fill_vec<EPC>(A[k], 1.f); fill_vec<EPC>(B[k], 0.f); fill_vec<EPC>(Cc[k], 0.f); }
    }
    const long stride = (long)nblk * 256;
    const long rounds = (total + stride - 1) / stride;
    const bool rev = p.exp & 2;
    auto body = [&](auto NTc) __attribute__((always_inline)) {
    constexpr bool LNT = decltype(NTc)::value;
    for (long rr = 0; rr < rounds; ++rr) {
        const long idx = walk_round(rr, rounds, rev) * stride + (long)bid * 256 + threadIdx.x;
        if (idx >= total) continue;
        const long off = idx * 16;
        float g[EPC];
        unpack16<T>(ld16<LNT>(p.dout + off), g);
        if (p.relu && p.mask) {
            mask_by_bits<EPC>(p.mask[idx], g);
        } else if (p.relu) {
            float o[EPC];
            unpack16<T>(ld16<LNT>(p.out + off), o);
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] = o[e] > 0.f ? g[e] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!p.dx[k]) continue;
            float r[EPC];
            if (p.x[k]) {
                float xv[EPC];
                unpack16<T>(ld16<LNT>(p.x[k] + off), xv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) r[e] = A[k][e] * g[e] + B[k][e] * xv[e] + Cc[k][e];
            } else {
#pragma unroll
                for (int e = 0; e < EPC; ++e) r[e] = g[e];
            }
            uint4* dst = reinterpret_cast<uint4*>(p.dx[k] + off);
            if (p.accumulate[k]) {
                float o[EPC];
                unpack16<T>(*dst, o);
#pragma unroll
                for (int e = 0; e < EPC; ++e) r[e] += o[e];
            }
            *dst = pack16<T>(r);
        }
    }
    };
    if (p.exp & 1) body(std::true_type{}); else body(std::false_type{});
    lh_l2_touch(p.touch, p.touch_bytes, bid, nblk);
}
};

struct fuse_bwd_coef_fused {
using Args = CoefArgs;
static __device__ __forceinline__ void run(const CoefArgs& p, const int bid, const int nblk) {
    const long count = p.count;
    const int c = p.c;
    auto fin = [&](int ch, double s0, double s1) {
        p.coef[ch] = (float)(s0 / (double)count);
        p.coef[c + ch] = (float)(s1 / (double)count);
        if (p.dbeta) p.dbeta[ch] = (float)s0;
        if (p.dgamma) p.dgamma[ch] = (float)s1;
    };
    if (p.rows >= LH_FOLD_WIDE_ROWS) slab_totals_then64(p.slab, p.rows, p.c, bid, fin);
    else slab_totals_then(p.slab, p.rows, p.c, bid, fin);
}
};

// Reduce / apply passes of DIFFERENT kinds in one grid (the terms of an HRNet exchange sum: BN terms without and with
// upsampling, identity terms): the kind is a per-problem tag next to the argument blocks.
struct KindTags { int k[LH_MULTI_MAX]; };
template <typename T>
__global__ __launch_bounds__(256) void fuse_bwd_reduce_mixed_kernel(const LhMulti<FuseBwdArgs> m, const KindTags kt) {
    int bid, nblk;
    const int i = lh_multi_pick(m, bid, nblk);
    switch (kt.k[i]) {
        case K_FB_REDUCE_GEN: fuse_bwd_reduce<T>::run(m.a[i], bid, nblk); break;
        case K_FB_REDUCE_FLAT: fuse_bwd_reduce_flat<T, false>::run(m.a[i], bid, nblk); break;
        default: fuse_bwd_reduce_flat<T, true>::run(m.a[i], bid, nblk); break;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void fuse_bwd_apply_mixed_kernel(const LhMulti<FuseBwdArgs> m, const KindTags kt) {
    int bid, nblk;
    const int i = lh_multi_pick(m, bid, nblk);
    switch (kt.k[i]) {
        case K_FB_APPLY_GEN: fuse_bwd_apply<T>::run(m.a[i], bid, nblk); break;
        case K_FB_APPLY_FLAT: fuse_bwd_apply_flat<T, false>::run(m.a[i], bid, nblk); break;
        default: fuse_bwd_apply_flat<T, true>::run(m.a[i], bid, nblk); break;
    }
}

// Strips of the streaming reduce pass = rows of the partial-sum slab the coefficient fold reads.  Measured on the R50 and
// HRNet-W32 steps: 512 strips for a node that runs alone (1 024: the fold is a longer latency chain, -0.08 ms per step
// for 512; 256: the reduce pass loses occupancy), 256 per node when several nodes share a launch (lh_fuse_bwd_multi;
// the caller says so in lh_fuse_bwd_desc.strips_cap, so that a node plans the same strips alone and in company).
static long fuse_bwd_strips(long count, int* rows_per_strip, int strips_cap = 0) {
    const long cap = strips_cap >= 16 && strips_cap <= 512 ? strips_cap : 512;
    long rps = (count + cap - 1) / cap;
    if (rps < 16) rps = 16;
    *rows_per_strip = (int)rps;
    return (count + rps - 1) / rps;
}

// bytes of ONE term's slice: partial slab + colsum scratch + totals (doubles) + coefficients, rounded to 256
static size_t fuse_bwd_term_bytes(int n, int h, int w, int c) {
    int rps;
    const long strips = fuse_bwd_strips((long)n * h * w, &rps);
    const size_t b = (size_t)strips * 2 * c * 4 + 16 + (size_t)(ceil_div(strips, 256) + 1) * 2 * c * 8 + (size_t)4 * c * 4;
    return (b + 255) & ~(size_t)255;
}

// every term of a node owns a slice of the workspace: the terms' passes are independent of each other and run as
// multi-problem launches (all reduce passes, then all coefficient folds, then all apply passes)
extern "C" size_t lh_fuse_bwd_workspace_bytes(int n, int h, int w, int c) { return 4 * fuse_bwd_term_bytes(n, h, w, c); }

// ---- launch records: a C-ABI call is first PLANNED into the kernel launches it consists of (kind, grid, phase, the
// argument block of that kind), then run phase by phase -- the records of a phase, of one call or of several independent
// calls, LH_MULTI_MAX per launch (multi.h).
struct BwdLaunch {
    int kind, grid;
    int phase;                   // 0 reduce, 1 coefficient fold, 2 apply (a pass only depends on the passes of lower phase)
    union {
        FuseBwdArgs fb;          // reduce and one-term apply kinds
        FuseBwd2Args fb2;        // K_FB_APPLY2
        CoefArgs co;             // K_FB_COEF
    };
    // the gradient buffers an apply record writes (null: that term's gradient is not wanted)
    void dsts(const void* out[2]) const {
        if (kind == K_FB_APPLY2) { out[0] = fb2.dx[0]; out[1] = fb2.dx[1]; }
        else { out[0] = fb.dx; out[1] = nullptr; }
    }
    // an apply record whose kernel ends with lh_l2_touch (the flat ones) takes the bytes to warm
    void set_touch(const void* p, size_t bytes) {
        if (kind == K_FB_APPLY2) { fb2.touch = (const unsigned char*)p; fb2.touch_bytes = (unsigned)bytes; }
        else if (kind == K_FB_APPLY_FLAT || kind == K_FB_APPLY_FLAT_X) { fb.touch = (const unsigned char*)p; fb.touch_bytes = (unsigned)bytes; }
    }
};

static int plan_fuse_bwd(const lh_fuse_bwd_desc* d, int n, int h, int w, int c, void* workspace, int dtype, std::vector<BwdLaunch>& v) {
    LH_REQUIRE(d && d->dout && d->nterms >= 1 && d->nterms <= 4, "lh_fuse_bwd: bad descriptor");
    LH_REQUIRE(!d->relu || d->out || d->relu_mask, "lh_fuse_bwd: relu needs the forward output or its mask bits");
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0 && c % (16 / es) == 0, "lh_fuse_bwd: c %d not a multiple of the 16-byte chunk", c);
    const int nchunk0 = c / (16 / es);
    const bool merge2 = d->nterms == 2 && d->log2up[0] == 0 && d->log2up[1] == 0 && (nchunk0 & (nchunk0 - 1)) == 0 &&
                        nchunk0 <= 256 && (d->dx[0] || d->dx[1]);
    const size_t term_bytes = fuse_bwd_term_bytes(n, h, w, c);
    FuseBwd2Args m2;
    m2.touch = nullptr; m2.touch_bytes = 0;
    if (merge2) {
        m2.dout = (const unsigned char*)d->dout; m2.out = (const unsigned char*)d->out; m2.c = c; m2.relu = d->relu;
        m2.mask = (const unsigned char*)d->relu_mask;
        for (int k = 0; k < 2; ++k) {
            m2.x[k] = (const unsigned char*)d->x[k]; m2.scale[k] = d->scale[k]; m2.mean[k] = d->save_mean[k];
            m2.invstd[k] = d->save_invstd[k]; m2.coef[k] = nullptr; m2.dx[k] = (unsigned char*)d->dx[k];
            m2.accumulate[k] = d->accumulate[k];
        }
    }
    if (merge2 && d->pre_partial) { m2.relu = 0; m2.out = nullptr; m2.mask = nullptr; }      // dout is the gated gradient already
    if (merge2) {
        m2.count = (long)n * h * w;
        for (int k = 0; k < 2; ++k) { m2.fold_slab[k] = nullptr; m2.fold_rows[k] = 0; m2.dgamma[k] = nullptr; m2.dbeta[k] = nullptr; }
    }
    for (int t = 0; t < d->nterms; ++t) {
        if (!d->dx[t]) continue;
        FuseBwdArgs a;
        a.fold_rows = 0;
        a.touch = nullptr; a.touch_bytes = 0;
        a.dout = (const unsigned char*)d->dout; a.out = (const unsigned char*)d->out;
        a.mask = (const unsigned char*)d->relu_mask;
        a.x = (const unsigned char*)d->x[t]; a.scale = d->scale[t]; a.mean = d->save_mean[t]; a.invstd = d->save_invstd[t];
        a.dx = (unsigned char*)d->dx[t]; a.dgamma = d->dgamma[t]; a.dbeta = d->dbeta[t];
        a.n = n; a.h = h; a.w = w; a.c = c; a.l = d->log2up[t]; a.relu = d->relu; a.accumulate = d->accumulate[t];
        LH_REQUIRE(a.l >= 0 && (h >> a.l) << a.l == h && (w >> a.l) << a.l == w, "lh_fuse_bwd: bad upsampling factor");
        a.count = (long)n * (h >> a.l) * (w >> a.l);
        a.partial = nullptr; a.totals = nullptr; a.coef = nullptr; a.rows_per_strip = 0;
        a.shift = nullptr;
        const int nchunk = c / (16 / es);
        const bool flat = a.l == 0 && (nchunk & (nchunk - 1)) == 0 && nchunk <= 256;
        // dout written by lh_igemm_gated: already the gated gradient, its partial sums come with it
        const bool two_bn = d->nterms == 2 && d->x[0] && d->x[1];
        const float* pre_slab = !(d->pre_partial && a.x) ? nullptr : (two_bn && t == 1) ? d->pre_partial2 : d->pre_partial;
        const bool pre = pre_slab != nullptr;
        if (d->pre_partial) {
            // one BatchNorm term under the ReLU, alone or with an identity term beside it (a residual tail, merged apply pass); or a tail
            // with a projection shortcut: two BatchNorm terms, each with its slab
            LH_REQUIRE((d->nterms == 1 || merge2) && d->relu && d->pre_rows >= 1 && a.l == 0 && (a.x || merge2) && (!two_bn || d->pre_partial2),
                       "lh_fuse_bwd: pre_partial takes a ReLU node with one BatchNorm term (alone, or beside one identity term) or a two-term tail with pre_partial2");
            a.relu = 0;
            a.out = nullptr; a.mask = nullptr;
        }
        // single BN term under the ReLU: the mask is sign(x*scale+shift), no need to read the stored activation
        a.mask_from_x = (!pre && flat && d->relu && d->nterms == 1 && a.x && d->shift[t]) ? 1 : 0;
        if (a.mask_from_x) a.shift = d->shift[t];
        a.total = a.count * (c / (16 / es));
        a.exp = bn_exp_flags() & 3;
        LH_REQUIRE((long)n * h * w * (c / (16 / es)) < (1L << 31), "lh_fuse_bwd: tensor too large for 32-bit chunk indices");
        if (a.x) {
            LH_REQUIRE(workspace && a.scale && a.mean && a.invstd, "lh_fuse_bwd: BN term %d lacks workspace/statistics", t);
            long strips = fuse_bwd_strips(a.count, &a.rows_per_strip, d->strips_cap);
            // small tensors (HRNet's branches): few enough strips that the apply pass folds them itself; a strip must stay
            // short (<= 64 KiB of the operand), else the reduce pass would lose the workgroups it streams with
            bool fold_in_apply = false;
            if (pre) {
                strips = d->pre_rows;
                fold_in_apply = flat && c <= 256 && getenv("LH_FOLD_IN_APPLY") == nullptr && strips * 2 * c <= LH_FOLD_IN_APPLY_FLOATS;
            } else if (flat && c <= 256 && getenv("LH_FOLD_IN_APPLY") == nullptr) {
                int rps2;
                const long s2 = fuse_bwd_strips(a.count, &rps2, (int)std::min<long>(d->strips_cap >= 16 ? d->strips_cap : 512, LH_FOLD_IN_APPLY_FLOATS / (2 * c)));
                if (s2 * 2 * c <= LH_FOLD_IN_APPLY_FLOATS && (long)rps2 * c * es <= 65536) {
                    fold_in_apply = true;
                    strips = s2;
                    a.rows_per_strip = rps2;
                }
            }
            a.partial = (float*)((unsigned char*)workspace + (size_t)t * term_bytes);
            const long slab_floats = pre ? 0 : strips * 2 * c;      // pre: the slab is the caller's, the workspace holds the scratch only
            double* scratch = (double*)(a.partial + ((slab_floats + 3) & ~3L));
            if (pre) a.partial = const_cast<float*>(pre_slab);
            double* totals = scratch + (long)ceil_div(strips, 256) * 2 * c;
            a.totals = totals;
            a.coef = (float*)(totals + 2 * c) + (size_t)(merge2 ? t : 0) * 2 * c;   // merging keeps one coefficient block per term
            if (!pre) {
                BwdLaunch r;
                r.kind = flat ? (a.mask_from_x ? K_FB_REDUCE_FLAT_X : K_FB_REDUCE_FLAT) : K_FB_REDUCE_GEN;
                r.grid = (int)strips;
                r.phase = 0;
                r.fb = a;
                v.push_back(r);
            }
            if (fold_in_apply) {
                if (merge2) { m2.fold_slab[t] = a.partial; m2.fold_rows[t] = (int)strips; m2.dgamma[t] = a.dgamma; m2.dbeta[t] = a.dbeta; }
                else a.fold_rows = (int)strips;
            } else {
                BwdLaunch q;
                q.phase = 1;
                q.kind = K_FB_COEF; q.grid = fold_grid((int)strips, c);
                q.co.slab = a.partial; q.co.rows = (int)strips; q.co.c = c; q.co.count = a.count; q.co.coef = a.coef; q.co.dgamma = a.dgamma; q.co.dbeta = a.dbeta;
                v.push_back(q);
            }
            if (merge2) m2.coef[t] = a.coef;
        }
        if (merge2) continue;                 // both gradients are written by ONE pass below
        BwdLaunch r;
        if (flat) {
            r.kind = a.mask_from_x ? K_FB_APPLY_FLAT_X : K_FB_APPLY_FLAT;
            r.grid = flat_grid(a.total);          // >= 4 chunks per thread
        } else {
            r.kind = K_FB_APPLY_GEN;
            r.grid = (int)((a.total + 255) / 256 > 4096 ? 4096 : (a.total + 255) / 256);
        }
        r.phase = 2;
        r.fb = a;
        v.push_back(r);
    }
    if (merge2) {
        BwdLaunch r;
        r.phase = 2;
        m2.total = (long)n * h * w * nchunk0;
        m2.exp = bn_exp_flags() & 3;
        r.kind = K_FB_APPLY2;
        r.grid = flat_grid(m2.total);
        r.fb2 = m2;
        v.push_back(r);
    }
    // the LAST launch of the call (an apply pass) warms what the next launch on the stream reads first (lh_fuse_bwd_desc.l2_touch)
    if (d->l2_touch && d->l2_touch_bytes > 0 && d->l2_touch_bytes < (1UL << 31) && !v.empty()) v.back().set_touch(d->l2_touch, d->l2_touch_bytes);
    return LH_OK;
}

// Run n <= LH_MULTI_MAX records of ONE kind: a plain launch for one, a multi-problem launch for several.
static int bn_run(const BwdLaunch* const* L, int n, int dtype, hipStream_t s) {
    LH_REQUIRE(n >= 1 && n <= LH_MULTI_MAX, "bn_run: %d records", n);
    switch (L[0]->kind) {
        case K_FB_REDUCE_GEN: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_reduce<T>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_REDUCE_FLAT: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_reduce_flat<T, false>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_REDUCE_FLAT_X: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_reduce_flat<T, true>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_COEF: lh_launch_records<fuse_bwd_coef_fused>(L, n, &BwdLaunch::co, s); break;
        case K_FB_APPLY_GEN: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_apply<T>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_APPLY_FLAT: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_apply_flat<T, false>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_APPLY_FLAT_X: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_apply_flat<T, true>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_APPLY2: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_apply2_flat<T>>(L, n, &BwdLaunch::fb2, s)); break;
        default: lh_set_error("bn_run: unknown kind %d", L[0]->kind); return LH_ERR_ARG;
    }
    LH_LAUNCH_CHECK("BatchNorm / ReLU pass launch");
    return LH_OK;
}

static int bn_run_mixed(const BwdLaunch* const* L, int n, int dtype, hipStream_t s) {
    LhMulti<FuseBwdArgs> m;
    KindTags kt;
    m.n = n; m.first[0] = 0;
    for (int i = 0; i < n; ++i) { m.a[i] = L[i]->fb; kt.k[i] = L[i]->kind; m.first[i + 1] = m.first[i] + L[i]->grid; }
    for (int i = n; i < LH_MULTI_MAX; ++i) kt.k[i] = 0;
    if (L[0]->phase == 0) { LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((fuse_bwd_reduce_mixed_kernel<T>), dim3(m.first[n]), dim3(256), 0, s, m, kt)); }
    else { LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((fuse_bwd_apply_mixed_kernel<T>), dim3(m.first[n]), dim3(256), 0, s, m, kt)); }
    LH_LAUNCH_CHECK("BatchNorm / ReLU mixed pass launch");
    return LH_OK;
}

// The backward passes of n planned calls, phase by phase (all reduce passes, all coefficient folds, all apply passes):
// inside a phase the passes are independent -- every term has its own workspace slice and its own gradient -- so they
// run LH_MULTI_MAX per launch, passes of one kind through that kind's kernel, the rest through the mixed kernels.
static int bn_run_phases(const std::vector<std::vector<BwdLaunch>>& plans, int dtype, hipStream_t s) {
    // two passes that write ONE gradient buffer (an activation that enters a node twice) must keep their recorded order
    std::vector<const void*> dsts;
    for (const auto& pl : plans)
        for (const BwdLaunch& r : pl) {
            if (r.phase != 2) continue;
            const void* d[2];
            r.dsts(d);
            for (const void* q : d) if (q) dsts.push_back(q);
        }
    std::sort(dsts.begin(), dsts.end());
    if (std::adjacent_find(dsts.begin(), dsts.end()) != dsts.end()) {
        const BwdLaunch* L[1];
        for (const auto& pl : plans)
            for (const BwdLaunch& r : pl) {
                L[0] = &r;
                const int rc = bn_run(L, 1, dtype, s);
                if (rc) return rc;
            }
        return LH_OK;
    }
    for (int phase = 0; phase < 3; ++phase) {
        std::vector<const BwdLaunch*> fbk, other;        // FuseBwdArgs reduce / apply passes | coefficient folds, two-term applies
        for (const auto& pl : plans)
            for (const BwdLaunch& r : pl) {
                if (r.phase != phase) continue;
                (r.kind == K_FB_COEF || r.kind == K_FB_APPLY2 ? other : fbk).push_back(&r);
            }
        // passes of one kind first (their own kernels, no kind switch), what is left over goes to the mixed kernel
        std::vector<const BwdLaunch*> rest;
        for (int kind = K_FB_REDUCE_GEN; kind <= K_FB_APPLY2; ++kind) {
            std::vector<const BwdLaunch*> same;
            for (const BwdLaunch* r : fbk) if (r->kind == kind) same.push_back(r);
            const size_t whole = same.size() / LH_MULTI_MAX * LH_MULTI_MAX;
            for (size_t i = 0; i < whole; i += LH_MULTI_MAX) {
                const int rc = bn_run(&same[i], LH_MULTI_MAX, dtype, s);
                if (rc) return rc;
            }
            rest.insert(rest.end(), same.begin() + whole, same.end());
        }
        for (size_t i = 0; i < rest.size(); i += LH_MULTI_MAX) {
            const int m = (int)(rest.size() - i < (size_t)LH_MULTI_MAX ? rest.size() - i : LH_MULTI_MAX);
            bool one = true;
            for (int k = 1; k < m; ++k) one = one && rest[i + k]->kind == rest[i]->kind;
            const int rc = one ? bn_run(&rest[i], m, dtype, s) : bn_run_mixed(&rest[i], m, dtype, s);
            if (rc) return rc;
        }
        for (int kind : {(int)K_FB_COEF, (int)K_FB_APPLY2}) {
            std::vector<const BwdLaunch*> same;
            for (const BwdLaunch* r : other) if (r->kind == kind) same.push_back(r);
            for (size_t i = 0; i < same.size(); i += LH_MULTI_MAX) {
                const int m = (int)(same.size() - i < (size_t)LH_MULTI_MAX ? same.size() - i : LH_MULTI_MAX);
                const int rc = bn_run(&same[i], m, dtype, s);
                if (rc) return rc;
            }
        }
    }
    return LH_OK;
}

extern "C" int lh_fuse_bwd(const lh_fuse_bwd_desc* d, int n, int h, int w, int c, void* workspace, int dtype,
                           void* stream) {
    std::vector<std::vector<BwdLaunch>> plans(1);
    const int rc = plan_fuse_bwd(d, n, h, w, c, workspace, dtype, plans[0]);
    if (rc) return rc;
    return bn_run_phases(plans, dtype, (hipStream_t)stream);
}

// n independent nodes (each with its OWN workspace): reduce / coefficient fold / apply of all of them as three launches.
extern "C" int lh_fuse_bwd_multi(const lh_fuse_bwd_call* calls, int n, int dtype, void* stream) {
    LH_REQUIRE(calls && n >= 1, "lh_fuse_bwd_multi: bad arguments");
    std::vector<std::vector<BwdLaunch>> plans(n);
    for (int i = 0; i < n; ++i) {
        const int rc = plan_fuse_bwd(calls[i].d, calls[i].n, calls[i].h, calls[i].w, calls[i].c, calls[i].workspace, dtype, plans[i]);
        if (rc) return rc;
    }
    return bn_run_phases(plans, dtype, (hipStream_t)stream);
}
