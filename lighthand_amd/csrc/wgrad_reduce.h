// The fold of a weight gradient's pixel-split slabs [split][tap][o][i] into the reference-layout gradient, deterministically and in
// split order: argument block, the two device bodies and the host-side preparation.  The __global__ kernels that wrap the bodies
// live in the unit that launches them (wgrad.hip: plain, contig, multi; wgrad_table.hip: table).
#pragma once
#include "common.h"

struct WreduceArgs {
    const float* slab;
    float* grad;
    int n_out, n_in, ntaps, nsplit, accumulate;
    int contig;                  // this problem folds on the transposing path (wgrad_reduce_contig_body); read by the table kernel only
    long so, si, sr, ss;
    signed char r[64];
    signed char s[64];
};

// Fast path for the plain layout grad[(o*n_in + i)*ntaps + t]: a workgroup folds 256 consecutive (o, i)
// pairs (coalesced slab reads per tap), transposes through LDS and writes 256*ntaps contiguous floats.
__device__ __forceinline__ void wgrad_reduce_contig_body(const WreduceArgs& p, float* tile, const int bid) {
    const long per = (long)p.n_out * p.n_in;
    const long base = (long)bid * 256;
    const long idx = base + threadIdx.x;
    const int ld = p.ntaps + 1;
    if (idx < per) {
        for (int t = 0; t < p.ntaps; ++t) {
            float a = 0.f;
            for (int sp = 0; sp < p.nsplit; ++sp) a += p.slab[((long)sp * p.ntaps + t) * per + idx];
            tile[threadIdx.x * ld + t] = a;
        }
    }
    __syncthreads();
    const long n_here = per - base < 256 ? per - base : 256;
    const long total = n_here * p.ntaps;
    float* g = p.grad + base * p.ntaps;
    for (long e = threadIdx.x; e < total; e += 256) {
        const int pair = (int)(e / p.ntaps), t = (int)(e - (long)pair * p.ntaps);
        const float v = tile[pair * ld + t];
        g[e] = p.accumulate ? g[e] + v : v;
    }
}

// Generic layout / small tensors: one thread per (tap, o, FOUR consecutive i) -- 16-byte coalesced slab reads, eight splits
// requested before the first is added (the fold is a latency chain over the splits), the sum itself strictly in split
// order; strided writes.  n_in not a multiple of 4: one element per thread.
static inline long wgrad_reduce_threads(long n_out, long n_in, long ntaps) {
    return (n_in & 3) == 0 ? n_out * n_in * ntaps / 4 : n_out * n_in * ntaps;
}
__device__ __forceinline__ void wgrad_reduce_body(const WreduceArgs& p, const int bid, const int nblk) {
    const long idx = (long)bid * blockDim.x + threadIdx.x;
    const long per = (long)p.n_out * p.n_in;
    if ((p.n_in & 3) == 0) {
        const long per4 = per >> 2;
        if (idx >= per4 * p.ntaps) return;
        // 32-bit index arithmetic: a weight tensor has far fewer than 2^31 elements (reduce_prepare checks)
        const unsigned iu = (unsigned)idx, p4 = (unsigned)per4;
        const int t = (int)(iu / p4);
        const unsigned pair4 = iu - (unsigned)t * p4;
        const unsigned n4 = (unsigned)p.n_in >> 2;
        const int o = (int)(pair4 / n4), i = (int)(pair4 - (unsigned)o * n4) * 4;
        const float4* src = reinterpret_cast<const float4*>(p.slab + (long)t * per + (long)o * p.n_in + i);
        const long stride = (long)p.ntaps * per4;          // float4 units between splits
        float4 a = float4{0.f, 0.f, 0.f, 0.f};
        int sp = 0;
        for (; sp + 8 <= p.nsplit; sp += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = float4(src[(long)(sp + u) * stride]);   // (the copy keeps the measured load addressing)
#pragma unroll
            for (int u = 0; u < 8; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
        }
        for (; sp < p.nsplit; ++sp) {
            const float4 v = src[(long)sp * stride];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        float* g = p.grad + o * p.so + i * p.si + p.r[t] * p.sr + p.s[t] * p.ss;
        const float r[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k * p.si] = p.accumulate ? g[k * p.si] + r[k] : r[k];
        return;
    }
    if (idx >= per * p.ntaps) return;
    const unsigned iu = (unsigned)idx, pu = (unsigned)per;
    const int t = (int)(iu / pu);
    const unsigned pair = iu - (unsigned)t * pu;
    const int o = (int)(pair / (unsigned)p.n_in), i = (int)(pair - (unsigned)o * (unsigned)p.n_in);
    float a = 0.f;
    const float* src = p.slab + (long)t * per + pair;
    const long stride = (long)p.ntaps * per;
    int sp = 0;
    for (; sp + 8 <= p.nsplit; sp += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(long)(sp + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; sp < p.nsplit; ++sp) a += src[(long)sp * stride];
    float* g = p.grad + o * p.so + i * p.si + p.r[t] * p.sr + p.s[t] * p.ss;
    *g = p.accumulate ? *g + a : a;
}

// Launch shape of one fold: workgroups of 256 threads, dynamic LDS (the transposing path's [256][ntaps + 1] tile).
static inline int wgrad_reduce_blocks(const WreduceArgs& r) {
    return r.contig ? ceil_div((long)r.n_out * r.n_in, 256) : ceil_div(wgrad_reduce_threads(r.n_out, r.n_in, r.ntaps), 256);
}
static inline int wgrad_reduce_lds(const WreduceArgs& r) { return r.contig ? 256 * (r.ntaps + 1) * (int)sizeof(float) : 0; }

// Check the arguments of the fold of one weight gradient with `nsplit` pixel splits (the caller's plan) and fill its argument block;
// contig = the transposing fast path applies.
static inline int reduce_prepare(const lh_igemm_desc* d, const float* slab, float* grad, int n_out, int n_in, long so, long si, long sr, long ss,
                                 const int* taps_rs, int accumulate, int nsplit, WreduceArgs* ap) {
    LH_REQUIRE(d && slab && grad && taps_rs, "lh_wgrad_reduce: null pointer");
    LH_REQUIRE(d->ntaps > 0 && d->ntaps <= 64, "lh_wgrad_reduce: ntaps %d out of range", d->ntaps);
    LH_REQUIRE((long)n_out * n_in * d->ntaps < (1L << 31), "lh_wgrad_reduce: weight tensor too large for 32-bit element indices");
    WreduceArgs& a = *ap;
    a.nsplit = nsplit;
    a.slab = slab; a.grad = grad; a.n_out = n_out; a.n_in = n_in; a.ntaps = d->ntaps;
    a.accumulate = accumulate; a.so = so; a.si = si; a.sr = sr; a.ss = ss;
    for (int t = 0; t < 64; ++t) {
        a.r[t] = t < d->ntaps ? (signed char)taps_rs[2 * t] : 0;
        a.s[t] = t < d->ntaps ? (signed char)taps_rs[2 * t + 1] : 0;
    }
    const long per = (long)n_out * n_in;
    bool contig = so == (long)n_in * d->ntaps && si == d->ntaps && ss == 1;
    for (int t = 0; t < d->ntaps && contig; ++t) contig = (a.r[t] * sr + a.s[t] * ss) == t;
    a.contig = contig && per * d->ntaps > (2L << 20);
    return LH_OK;
}
