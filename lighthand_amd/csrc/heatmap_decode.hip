// Heat-map decode: hard arg-max, quarter-pixel refinement, DARK, flip-test merge with arg-max, soft-arg-max.
#include <cmath>
#include "common.h"
#include "heatmap_reduce.h"

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
    argmax_finish(best, have, red, w, scale, preds, maxvals, idx);
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
//      which only the maximum over the plane is kept (block_max);
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
    bmax = block_max(bmax, red);
    if (tid < 13) {
        // stencil points: 0..4 = (px-2 .. px+2, py), 5..8 = (px, py-2), (px, py-1), (px, py+1), (px, py+2), 9..12 = the diagonals
        // (-1,-1), (+1,-1), (-1,+1), (+1,+1); all inside the plane by the skip test
        int ox, oy;
        if (tid < 5) { ox = tid - 2; oy = 0; }
        else if (tid < 9) { ox = 0; oy = tid < 7 ? tid - 7 : tid - 6; }
        else { ox = (tid - 9) & 1 ? 1 : -1; oy = tid < 11 ? -1 : 1; }
        const float s = maxval / bmax;
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
    argmax_finish(best, have, red, w, scale, preds, maxvals, idx);
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
    mx = block_max(mx, rmax);
    double s0 = 0.0, sx = 0.0, sy = 0.0;
    for (int i = threadIdx.x; i < hw; i += 256) {
        const double e = (double)expf(beta * (m[i] - mx));
        s0 += e; sx += e * (double)(i % w); sy += e * (double)(i / w);
    }
    const Moments t = block_sum_moments(s0, sx, sy, rs);
    if (threadIdx.x == 0) {
        preds[blockIdx.x * 2 + 0] = (float)(t.sx / t.s0) * scale;
        preds[blockIdx.x * 2 + 1] = (float)(t.sy / t.s0) * scale;
    }
}

extern "C" int lh_heatmap_soft_argmax(const float* heatmaps, int bj, int h, int w, float beta, float scale, float* preds,
                                      void* stream) {
    LH_REQUIRE(heatmaps && preds && bj > 0 && h > 0 && w > 0, "lh_heatmap_soft_argmax: bad arguments");
    hipLaunchKernelGGL(heatmap_soft_argmax_kernel, dim3(bj), dim3(256), 0, (hipStream_t)stream, heatmaps, h * w, w, beta, scale, preds);
    LH_LAUNCH_CHECK("heatmap_soft_argmax launch");
    return LH_OK;
}
