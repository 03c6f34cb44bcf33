// Device side of the fused op's backward (fuse_bwd.hip): the argument blocks, the helpers the passes share, the passes --
// reduce (partial sums of g and g * xhat), coefficient fold, apply -- and the coefficient fold an apply pass runs itself.
#pragma once
#include "bn_common.h"
#include "multi.h"
#include <type_traits>

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
    float* coef;                 // [2][c]: mean(g), mean(g*xhat)
    float* dgamma;
    float* dbeta;
    int h, w, c;                 // OUTPUT resolution
    int l, relu, accumulate;
    const float* shift;          // the *_X kinds: ReLU mask recomputed from x*scale+shift (single BN term), `out` is not read
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

// ---- what the passes share.  Per-thread arrays go in by reference-to-array, and store_grad adds into a copy, not into its
// caller's array: with decayed pointers, or the addition in place, the same arithmetic compiled to 6-12 more VGPRs in the
// 16-bit flat applies (a wave of occupancy) and to up to 114 more instructions.
// The ReLU gate of one chunk of the incoming gradient: by the sign of x*scale+shift (MASK_X), by the mask bits, or by the
// stored output.  mbits() / outv() fetch the mask byte / the 16 bytes of `out` -- only the source in use is called.
template <typename T, bool MASK_X, class MB, class OV>
__device__ __forceinline__ void gate_grad(int relu, bool has_mask, const float* xv, const float* sc, const float* sh, MB&& mbits, OV&& outv, float (&g)[16 / sizeof(T)]) {
    constexpr int EPC = 16 / sizeof(T);
    if (MASK_X) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) g[e] = (xv[e] * sc[e] + sh[e]) > 0.f ? g[e] : 0.f;
    } else if (relu) {
        if (has_mask) {
            mask_by_bits<EPC>(mbits(), g);
        } else {
            float o[EPC];
            unpack16<T>(outv(), o);
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] = o[e] > 0.f ? g[e] : 0.f;
        }
    }
}

// cell r of a [n][hs][ws] map -> (n, ys, xs).  32-bit: count < 2^31 (plan_fuse_bwd)
__device__ __forceinline__ void split_cell(unsigned r, int hs, int ws, int& n, int& ys, int& xs) {
    const unsigned t2 = r / (unsigned)ws;
    xs = (int)(r - t2 * (unsigned)ws);
    n = (int)(t2 / (unsigned)hs);
    ys = (int)(t2 - (unsigned)n * (unsigned)hs);
}

// optionally add what is in dx, pack, store
template <typename T> __device__ __forceinline__ void store_grad(unsigned char* dx, int accumulate, const float (&g)[16 / sizeof(T)]) {
    constexpr int EPC = 16 / sizeof(T);
    uint4* dst = reinterpret_cast<uint4*>(dx);
    float r[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) r[e] = g[e];
    if (accumulate) {
        float o[EPC];
        unpack16<T>(*dst, o);
#pragma unroll
        for (int e = 0; e < EPC; ++e) r[e] += o[e];
    }
    *dst = pack16<T>(r);
}

// The strip's sums of nc chunks from every thread's s1 / s2 (thread = row lane k * nc + chunk cl) to its slab row:
// out[0..) = sum g, out[c..) = sum g * xhat, the row lanes added in ascending order.
template <int EPC>
__device__ __forceinline__ void store_strip_sums(float* red, const float (&s1)[EPC], const float (&s2)[EPC], int nc, int lanes, int c, float* out) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) { red[(threadIdx.x * EPC + e) * 2] = s1[e]; red[(threadIdx.x * EPC + e) * 2 + 1] = s2[e]; }
    __syncthreads();
    for (int t = threadIdx.x; t < nc * EPC; t += 256) {
        const int cl = t / EPC, e = t % EPC;
        float a = 0.f, b = 0.f;
        for (int k = 0; k < lanes; ++k) { a += red[((k * nc + cl) * EPC + e) * 2]; b += red[((k * nc + cl) * EPC + e) * 2 + 1]; }
        out[cl * EPC + e] = a;
        out[c + cl * EPC + e] = b;
    }
}

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
            gate_grad<T, false>(p.relu, p.mask != nullptr, nullptr, nullptr, nullptr, [&] { return (unsigned)p.mask[off >> 4]; },
                                [&] { return *reinterpret_cast<const uint4*>(p.out + off); }, d);
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] += d[e];
        }
}

// Coefficient fold INSIDE the apply pass (small tensors only, plan_fuse_bwd): every workgroup folds the reduce pass's
// [rows][2][c] partial sums itself -- rows * 2c <= 16 Ki floats, all of its loads in flight at once, fp64 sums in a fixed
// order, so every workgroup gets bit-identical coefficients -- and the separate fold launch (5-6 us on the dependency chain
// of every BatchNorm of HRNet's branches) disappears.  coefL[0..c) = mean(g), coefL[c..2c) = mean(g * xhat); workgroup 0
// also stores the parameter gradients dbeta = sum(g), dgamma = sum(g * xhat).
constexpr int LH_FOLD_IN_APPLY_FLOATS = 16384;
// rows r0, r0 + step, ... of one column, eight of them in flight, added in ascending order
__device__ __forceinline__ double fold_column(const float* slab, int ncol, int col, int r0, int step, int rows) {
    double a = 0.0;
    int r = r0;
    for (; r + 7 * step < rows; r += 8 * step) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = slab[(long)(r + u * step) * ncol + col];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += (double)v[u];
    }
    for (; r < rows; r += step) a += (double)slab[(long)r * ncol + col];
    return a;
}
__device__ __forceinline__ void fold_coef_block(const float* slab, int rows, int c, long count, float* dgamma, float* dbeta,
                                                bool writer, float* coefL) {
    __shared__ double fold_part[512];
    const int ncol = 2 * c;                              // power of two, <= 512
    const int t = threadIdx.x;
    auto finish = [&](int col, double tot) {
        coefL[col] = (float)(tot / (double)count);
        if (writer) {
            if (col < c) { if (dbeta) dbeta[col] = (float)tot; }
            else if (dgamma) dgamma[col - c] = (float)tot;
        }
    };
    if (ncol <= 256) {
        const int parts = 256 / ncol;
        fold_part[t] = fold_column(slab, ncol, t & (ncol - 1), t / ncol, parts, rows);
        __syncthreads();
        if (t < ncol) {
            double tot = 0.0;
            for (int q = 0; q < parts; ++q) tot += fold_part[q * ncol + t];
            finish(t, tot);
        }
    } else {                                             // 2c = 512: two columns per thread, every row
#pragma unroll
        for (int h = 0; h < 2; ++h) finish(t + 256 * h, fold_column(slab, ncol, t + 256 * h, 0, 1, rows));
    }
    __syncthreads();
}

// One BatchNorm or identity term as an apply pass sees it: of FuseBwdArgs, or term k of FuseBwd2Args.
struct TermView {
    const unsigned char* x;      // null: identity
    const float* scale;
    const float* invstd;
    const float* mean;
    const float* coef;           // [2][c] from the coefficient launch, or
    const float* fold_slab;      // non-null: the workgroup folds fold_slab[fold_rows][2][c] itself (fold_coef_block)
    int fold_rows;
    float* dgamma;
    float* dbeta;
};
__device__ __forceinline__ TermView term_view(const FuseBwdArgs& p) {
    return {p.x, p.scale, p.invstd, p.mean, p.coef, p.fold_rows > 0 ? p.partial : nullptr, p.fold_rows, p.dgamma, p.dbeta};
}
__device__ __forceinline__ TermView term_view(const FuseBwd2Args& p, int k) {
    return {p.x[k], p.scale[k], p.invstd[k], p.mean[k], p.coef[k], p.fold_slab[k], p.fold_rows[k], p.dgamma[k], p.dbeta[k]};
}

// The term's dx = scale*(g - c0 - xhat*c1) = A*g + B*x + C  with  xhat = (x - mean)*invstd, for this thread's channel chunk
// (A = scale).  c0 / c1 come from the coefficient launch or from this workgroup's own fold through coefL (LDS, 512 floats;
// sync_first: coefL still holds what another term's threads may be reading; workgroup 0 writes dgamma / dbeta).
// Identity term: dx = g.
template <int EPC>
__device__ __forceinline__ void term_coefs(const TermView& t, int c, long count, int bid, bool sync_first, float* coefL, int chunk,
                                           float (&A)[EPC], float (&B)[EPC], float (&Cc)[EPC]) {
    if (!t.x) { fill_vec<EPC>(A, 1.f); fill_vec<EPC>(B, 0.f); fill_vec<EPC>(Cc, 0.f); return; }
    float iv[EPC], c0[EPC], c1[EPC], mn[EPC];
    load_vec<EPC>(t.scale + chunk * EPC, A);
    load_vec<EPC>(t.invstd + chunk * EPC, iv);
    if (t.fold_slab) {
        if (sync_first) __syncthreads();
        fold_coef_block(t.fold_slab, t.fold_rows, c, count, t.dgamma, t.dbeta, bid == 0, coefL);
#pragma unroll
        for (int e = 0; e < EPC; ++e) { c0[e] = coefL[chunk * EPC + e]; c1[e] = coefL[c + chunk * EPC + e]; }
    } else {
        load_vec<EPC>(t.coef + chunk * EPC, c0);
        load_vec<EPC>(t.coef + c + chunk * EPC, c1);
    }
    load_vec<EPC>(t.mean + chunk * EPC, mn);
#pragma unroll
    for (int e = 0; e < EPC; ++e) { B[e] = -A[e] * iv[e] * c1[e]; Cc[e] = -A[e] * c0[e] - B[e] * mn[e]; }
}

// ---- the passes
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
                int n, ys, xs;
                split_cell((unsigned)r, hs, ws, n, ys, xs);
                float g[EPC], xv[EPC];
                cell_grad<T, EPC>(p, n, ys, xs, chunk, g);
                unpack16<T>(*reinterpret_cast<const uint4*>(p.x + (r * p.c + chunk * EPC) * sizeof(T)), xv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) { s1[e] += g[e]; s2[e] += g[e] * (xv[e] - mean[e]) * inv[e]; }
            }
        }
        store_strip_sums<EPC>(red, s1, s2, nc, lanes, p.c, out + cb * EPC);
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
        int n, ys, xs;
        split_cell(r, hs, ws, n, ys, xs);
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
        store_grad<T>(p.dx + idx * 16, p.accumulate, g);
    }
}
};

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
        gate_grad<T, MASK_X>(p.relu, p.mask != nullptr, xv, sc, sh, [&] { return mbits; }, [&] { return od; }, g);
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
    store_strip_sums<EPC>(red, s1, s2, nchunk, lanes, p.c, p.partial + (long)bid * 2 * p.c);
}
};

template <typename T, bool MASK_X> struct fuse_bwd_apply_flat {
using Args = FuseBwdArgs;
static __device__ __forceinline__ void run(const FuseBwdArgs& p, const int bid, const int nblk) {
    const long total = p.total;
    constexpr int EPC = 16 / sizeof(T);
    const int nchunk = p.c / EPC;
    const int chunk = threadIdx.x & (nchunk - 1);
    __shared__ float coefL[512];
    float A[EPC], B[EPC], Cc[EPC], sh[EPC];
    term_coefs<EPC>(term_view(p), p.c, p.count, bid, false, coefL, chunk, A, B, Cc);
    if (MASK_X && p.x) load_vec<EPC>(p.shift + chunk * EPC, sh);       // the gate's scale is A
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
        gate_grad<T, MASK_X>(p.relu, p.mask != nullptr, xv, A, sh, [&] { return (unsigned)p.mask[off >> 4]; }, [&] { return ld16<LNT>(p.out + off); }, g);
        if (p.x) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) g[e] = A[e] * g[e] + B[e] * xv[e] + Cc[e];
        }
        store_grad<T>(p.dx + off, p.accumulate, g);
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
    __shared__ float coefL2[512];
    float A[2][EPC], B[2][EPC], Cc[2][EPC];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        term_coefs<EPC>(term_view(p, k), p.c, p.count, bid, k != 0, coefL2, chunk, A[k], B[k], Cc[k]);      // k: the other term's coefficients have been read by every thread
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
        gate_grad<T, false>(p.relu, p.mask != nullptr, nullptr, nullptr, nullptr, [&] { return (unsigned)p.mask[idx]; }, [&] { return ld16<LNT>(p.out + off); }, g);
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
            store_grad<T>(p.dx[k] + off, p.accumulate[k], r);
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
