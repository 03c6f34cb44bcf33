// Block reductions of the heat-map kernels (heatmap_loss.hip, heatmap_decode.hip).  Every function assumes a 256-thread workgroup
// (four waves of 64), takes its four LDS slots from the caller, holds one barrier that all 256 threads must reach, and returns the
// same value to every thread.  Fixed order -- wave-64 xor butterfly, one slot per wave, the slots combined as written -- and no
// atomics, so every replay gives the same bits.
#pragma once
#include <cmath>
#include "common.h"

// fp64 sum: red[0] + red[1] + red[2] + red[3]
__device__ __forceinline__ double block_sum(double acc, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// fp32 maximum (fmaxf: a NaN operand is dropped)
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// the three fp64 sums of a soft-arg-max: S0 = sum e, Sx = sum e x, Sy = sum e y; slot rs[wave] = {s0, sx, sy}, each summed left to right
struct Moments { double s0, sx, sy; };
__device__ __forceinline__ Moments block_sum_moments(double s0, double sx, double sy, double (*rs)[3]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o); }
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6][0] = s0; rs[threadIdx.x >> 6][1] = sx; rs[threadIdx.x >> 6][2] = sy; }
    __syncthreads();
    return Moments{rs[0][0] + rs[1][0] + rs[2][0] + rs[3][0], rs[0][1] + rs[1][1] + rs[2][1] + rs[3][1],
                   rs[0][2] + rs[1][2] + rs[2][2] + rs[3][2]};
}

struct Cand { float v; int i; };
// true when a precedes b under numpy.argmax's rule: NaN beats everything, then larger value,
// ties (and NaN vs NaN) broken by the lower flat index.
__device__ __forceinline__ bool cand_before(const Cand& a, const Cand& b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an || bn) return an && (!bn || a.i < b.i);
    return a.v > b.v || (a.v == b.v && a.i < b.i);
}

// The end of an arg-max over plane blockIdx.x of width w: `best` is the thread's candidate over its elements, `have` whether it saw
// any (index 0x7fffffff marks "none", so a plane smaller than the workgroup is decoded from the threads that hold an element).
// Thread 0 stores get_max_preds' outputs: the peak's (x, y) * scale, zeroed unless the maximum is > 0, the maximum, and its flat
// index when idx is given.
__device__ __forceinline__ void argmax_finish(Cand best, bool have, Cand* red, int w, float scale, float* preds, float* maxvals,
                                              int* idx) {
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
