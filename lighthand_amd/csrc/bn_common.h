// What more than one of the BatchNorm / ReLU / pool units (bn_stats.hip, fuse_fwd.hip, fuse_bwd.hip, pool.hip) needs: the
// slab folds, the cache-policy switches, the ReLU mask bits, per-channel vector loads and the grids of the streaming passes.
// All of them HBM-bound NHWC kernels: one 16-byte chunk (8 x 16-bit or 4 x fp32 channels) per lane, per-channel vectors in fp32.
#pragma once
#include "common.h"
#include "bn_fold.h"
#include <stdlib.h>

#ifndef LH_BN_EXP_DEFAULT
#define LH_BN_EXP_DEFAULT 4      // measured (round 4): non-temporal loads of the BN inputs in the forward pass, -0.11 ms per R50 step
#endif

// One workgroup = 16 channels x 16 row lanes: totals of the sum / sum-of-squares (or g / g*xhat) columns of a
// [rows][2][c] slab, handed to a per-channel functor by the first 16 threads (no second launch).
template <typename TI, typename F>
__device__ __forceinline__ void slab_totals_then(const TI* slab, int rows, int c, int bid, F&& fin) {
    __shared__ double red[2][16][17];
    const int ch = bid * 16 + (threadIdx.x & 15), rl = threadIdx.x >> 4;
    double a = 0.0, b = 0.0;
    if (ch < c) slab_lane16(slab, rows, c, ch, rl, [](const TI* q) { return *q; }, a, b);
    red[0][rl][threadIdx.x & 15] = a;
    red[1][rl][threadIdx.x & 15] = b;
    __syncthreads();
    if (threadIdx.x < 16 && ch < c) {
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s0 += red[0][i][threadIdx.x]; s1 += red[1][i][threadIdx.x]; }
        fin(ch, s0, s1);
    }
}

// The same totals with 4 channels x 64 row lanes per workgroup, for slabs of >= 256 rows: four times the workgroups and a
// quarter of the rows per lane (the fold kernels sit on the dependency chain of every BatchNorm: their length is a
// latency chain of row loads, 16 deep at 1 024 rows with 16 lanes, 4 deep with 64).  Lanes of a wave that share a channel
// fold by shuffles, the four waves through LDS, in a fixed order.
template <typename TI, typename F>
__device__ __forceinline__ void slab_totals_then64(const TI* slab, int rows, int c, int bid, F&& fin) {
    __shared__ double red64[2][4][4];
    const int ch = bid * 4 + (threadIdx.x & 3), rl = threadIdx.x >> 2;
    double a = 0.0, b = 0.0;
    if (ch < c) {
        int r = rl;
        for (; r + 448 < rows; r += 512) {        // eight independent row groups in flight (the fold is a latency chain)
            TI av[8], bv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { av[u] = slab[((long)(r + 64 * u) * 2) * c + ch]; bv[u] = slab[((long)(r + 64 * u) * 2 + 1) * c + ch]; }
            a += (((double)av[0] + (double)av[1]) + ((double)av[2] + (double)av[3])) + (((double)av[4] + (double)av[5]) + ((double)av[6] + (double)av[7]));
            b += (((double)bv[0] + (double)bv[1]) + ((double)bv[2] + (double)bv[3])) + (((double)bv[4] + (double)bv[5]) + ((double)bv[6] + (double)bv[7]));
        }
        for (; r + 192 < rows; r += 256) {        // four independent row groups in flight
            const TI a0 = slab[((long)r * 2) * c + ch], b0 = slab[((long)r * 2 + 1) * c + ch];
            const TI a1 = slab[((long)(r + 64) * 2) * c + ch], b1 = slab[((long)(r + 64) * 2 + 1) * c + ch];
            const TI a2 = slab[((long)(r + 128) * 2) * c + ch], b2 = slab[((long)(r + 128) * 2 + 1) * c + ch];
            const TI a3 = slab[((long)(r + 192) * 2) * c + ch], b3 = slab[((long)(r + 192) * 2 + 1) * c + ch];
            a += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
            b += ((double)b0 + (double)b1) + ((double)b2 + (double)b3);
        }
        for (; r < rows; r += 64) {
            a += (double)slab[((long)r * 2) * c + ch];
            b += (double)slab[((long)r * 2 + 1) * c + ch];
        }
    }
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < 4) { red64[0][wave][lane] = a; red64[1][wave][lane] = b; }
    __syncthreads();
    if (threadIdx.x < 4 && ch < c) {
        const double s0 = ((red64[0][0][threadIdx.x] + red64[0][1][threadIdx.x]) + red64[0][2][threadIdx.x]) + red64[0][3][threadIdx.x];
        const double s1 = ((red64[1][0][threadIdx.x] + red64[1][1][threadIdx.x]) + red64[1][2][threadIdx.x]) + red64[1][3][threadIdx.x];
        fin(ch, s0, s1);
    }
}

constexpr int LH_FOLD_WIDE_ROWS = 256;        // slabs with at least this many rows use the 64-lane fold (grid = c / 4)
static inline int fold_grid(int rows, int c) { return rows >= LH_FOLD_WIDE_ROWS ? ceil_div(c, 4) : ceil_div(c, 16); }

// ------------------------------------------------------------------------------------------------
// Cache-policy / traversal experiments of the streaming BN passes (LH_BN_EXP, read once per process; speed only, results
// do not depend on it): bit 0 = non-temporal loads for the LAST-USE reads of the backward apply passes (dout, x, out),
// bit 1 = the apply passes walk the tensor back to front (what the reduce pass read last is re-read first), bit 2 =
// non-temporal loads of the BN inputs in the forward pass, bit 3 = the forward pass walks back to front (the tail of the
// convolution's output, written last, is read first).
static int bn_exp_flags() {
    static const int v = [] { const char* e = getenv("LH_BN_EXP"); return e ? atoi(e) : LH_BN_EXP_DEFAULT; }();
    return v;
}
typedef unsigned int lh_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ uint4 ld16(const unsigned char* p) {
    if constexpr (NT) {
        const lh_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const lh_u32x4*>(p));
        return uint4{v[0], v[1], v[2], v[3]};
    } else {
        return *reinterpret_cast<const uint4*>(p);
    }
}
// index of round r of a grid-stride walk over `rounds` rounds, front to back or back to front
__device__ __forceinline__ long walk_round(long r, long rounds, bool rev) { return rev ? rounds - 1 - r : r; }

// L2 warm-up at the tail of an elementwise pass (round 5, profiles/r05_ingest_ladder.txt sitting 6): the convolution that follows on
// the stream walks its weight pack stage by stage in every workgroup at once, so each stage waits for lines no XCD has seen yet (the
// complete K loop of the stage-3 3x3: 21.3 us, 19.1 us with the pack already in L2).  L2 contents survive the kernel boundary: the
// workgroups that share an XCD (ids b, b + 8, ...) read one 4-byte word of every 128-byte line of the pack between them, right
// before they end.  Speed only: nothing depends on the values.
__device__ __forceinline__ void lh_l2_touch(const unsigned char* p, unsigned bytes, int bid, int nblk) {
    if (!p) return;
    const int per_xcd = nblk >> 3, idx = bid >> 3;
    if (idx >= per_xcd) return;
    const unsigned lines = bytes >> 7;
    unsigned acc = 0;
    for (unsigned l = (unsigned)idx * 256u + threadIdx.x; l < lines; l += (unsigned)per_xcd * 256u)
        acc ^= *reinterpret_cast<const unsigned*>(p + ((unsigned long)l << 7));
    asm volatile("" ::"v"(acc));
}

// The ReLU mask byte of a 16-byte chunk, written by the forward pass (positive_bits) and read by the backward passes (mask_by_bits).
// bit e of the result = (stored element e > 0): computed from the ROUNDED values so that it equals `out > 0`
template <typename T> __device__ __forceinline__ unsigned char positive_bits(const uint4& u) {
    constexpr int EPC = 16 / sizeof(T);
    float r[EPC];
    unpack16<T>(u, r);
    unsigned m = 0;
#pragma unroll
    for (int e = 0; e < EPC; ++e) m |= (r[e] > 0.f ? 1u : 0u) << e;
    return (unsigned char)m;
}
template <int EPC> __device__ __forceinline__ void mask_by_bits(unsigned m, float* g) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) g[e] = ((m >> e) & 1u) ? g[e] : 0.f;
}

// EPC consecutive floats of a per-channel vector with 16-byte loads.
template <int EPC> __device__ __forceinline__ void load_vec(const float* p, float* dst) {
#pragma unroll
    for (int q = 0; q < EPC / 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(p)[q];
        dst[4 * q] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
    }
}
template <int EPC> __device__ __forceinline__ void fill_vec(float* dst, float v) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) dst[e] = v;
}

// The flat passes of fuse_fwd.hip / fuse_bwd.hip keep ONE channel chunk per thread: the chunks of a pixel must divide the
// 256 threads of a workgroup.
static inline bool bn_flat_chunks(int nchunk) { return (nchunk & (nchunk - 1)) == 0 && nchunk <= 256; }

// streaming grid of the flat passes: one workgroup per 4 x 256 chunks, at most 2048 workgroups (re-measured in round 3:
// 1024 / 4096 workgroups, 2 / 8 chunks per thread: 9.60-9.66 ms against 9.61, 8 chunks 9.72)
static int flat_grid(long total) {
    const long g = (total + 1023) / 1024;
    return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
}
// grid of the generic (grid-stride) passes: one chunk per thread, at most 4096 workgroups
static int generic_grid(long total) {
    const long g = (total + 255) / 256;
    return (int)(g > 4096 ? 4096 : g);
}

// the bytes lh_l2_touch takes from a descriptor's l2_touch / l2_touch_bytes: a 32-bit count, 0 = nothing to warm
static inline unsigned lh_touch_bytes(const void* p, size_t bytes) { return p && bytes < (1UL << 31) ? (unsigned)bytes : 0u; }
