// Image ingest: float and uint8 (resize, ColorJitter, affine warp) images to padded NHWC4, keypoint warp, mirror, NHWC <-> NCHW.
#include "common.h"
#include "color_jitter.h"

// ------------------------------------------------------------------------------------------------ transforms
template <typename T>
__global__ void image_to_nhwc4_kernel(const float* src, T* dst, int n, int h, int w, int pad, int hp, int wp) {
    // 32-bit index arithmetic (the launcher checks n * hp * wp < 2^31: the 64-bit divisions were most of this kernel's instructions)
    // and one store per pixel
    const unsigned total = (unsigned)n * hp * wp;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned t = i / (unsigned)wp;
        const int x = (int)(i - t * (unsigned)wp);
        const int b = (int)(t / (unsigned)hp), y = (int)(t - (unsigned)b * (unsigned)hp);
        const int sy = y - pad, sx = x - pad;
        float v[3] = {0.f, 0.f, 0.f};
        if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {
            const long base = ((long)b * 3 * h + sy) * w + sx;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = src[base + (long)c * h * w];
        }
        if constexpr (sizeof(T) == 2) {
            union { uint2 u; T e[4]; } pk;
            pk.e[0] = from_f<T>(v[0]); pk.e[1] = from_f<T>(v[1]); pk.e[2] = from_f<T>(v[2]); pk.e[3] = from_f<T>(0.f);
            *reinterpret_cast<uint2*>(dst + (long)i * 4) = pk.u;
        } else {
            T* o = dst + (long)i * 4;
            o[0] = from_f<T>(v[0]); o[1] = from_f<T>(v[1]); o[2] = from_f<T>(v[2]); o[3] = from_f<T>(0.f);
        }
    }
}

extern "C" int lh_image_to_nhwc4(const float* nchw, void* out, int n, int h, int w, int pad, int wp, int dtype,
                                 void* stream) {
    LH_REQUIRE(nchw && out && n > 0 && h > 0 && w > 0 && pad >= 0 && wp >= w + 2 * pad, "lh_image_to_nhwc4: bad arguments");
    const int hp = h + 2 * pad;
    const long total = (long)n * hp * wp;
    LH_REQUIRE(total < (1L << 31), "lh_image_to_nhwc4: image batch too large for 32-bit pixel indices");
    const int grid = lh_grid(total, 8192);
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((image_to_nhwc4_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream,
                                                   nchw, (T*)out, n, h, w, pad, hp, wp));
    LH_LAUNCH_CHECK("image_to_nhwc4 launch");
    return LH_OK;
}

// Fused input pipeline: uint8 HWC image -> ToTensor (/255) -> bilinear Resize(h, w)
// (half-pixel centres, no antialias: torchvision's tensor Resize when upsampling 224 -> 256) -> Normalize(mean, std)
// -> zero-padded NHWC4 in the run dtype.  Reference CPU path: src/tools/dataset.py:128-159.
struct U8Args {
    const unsigned char* src;
    void* dst;
    int n, hs, ws, h, w, pad, hp, wp;
    float mean[3], istd[3];
};

// ---- the same pipeline with torchvision's ColorJitter between Resize and Normalize (src/tools/dataset.py:134-146).
// The random draw stays on the host (ColorJitter.get_params): per image four factors (brightness, contrast,
// saturation, hue) and the op order (four op ids 0..3, negative = skip) arrive as device arrays.  Contrast blends
// with the mean grey level of the WHOLE image as it is when the op runs, so a first kernel reduces that mean (of the
// image after the ops that precede contrast) into fp64 strip sums, and the second kernel applies everything.
// The four ops and cj_apply: color_jitter.h, shared with the frame crop (frames_crop_kernel.h).
__device__ __forceinline__ void u8_bilinear(const U8Args& p, int b, int oy, int ox, float* c) {
    const float sy = (float)p.hs / p.h, sx = (float)p.ws / p.w;
    float fy = (oy + 0.5f) * sy - 0.5f, fx = (ox + 0.5f) * sx - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + 1 < p.hs ? y0 + 1 : p.hs - 1, x1 = x0 + 1 < p.ws ? x0 + 1 : p.ws - 1;
    const float wy = fy - y0, wx = fx - x0;
    const unsigned char* base = p.src + (long)b * p.hs * p.ws * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a00 = base[((long)y0 * p.ws + x0) * 3 + ch], a01 = base[((long)y0 * p.ws + x1) * 3 + ch];
        const float a10 = base[((long)y1 * p.ws + x0) * 3 + ch], a11 = base[((long)y1 * p.ws + x1) * 3 + ch];
        const float top = a00 + (a01 - a00) * wx, bot = a10 + (a11 - a10) * wx;
        c[ch] = (top + (bot - top) * wy) * (1.f / 255.f);
    }
}

// Per-image affine warp in front of the resize (lh_image_u8_warp_to_nhwc4): output pixel (ox, oy) of the h x w frame samples
// the resized frame at u = inv[b] . (ox, oy, 1), both in output pixel-index coordinates (pixel centres on the integers).
// Inside [-0.5, w-0.5] x [-0.5, h-0.5] the sample is u8_bilinear's resize rule at u; outside the pixel is black (0 before
// ColorJitter and Normalize: cv2.warpAffine's constant border).  The matrix is applied before the resize arithmetic, so the
// identity gives ux = 1*ox + 0*oy + 0 = ox exactly and the plain kernels' output bit for bit (-ffp-contract=off).
__device__ __forceinline__ void u8_warp_bilinear(const U8Args& p, const float* inv, int b, int oy, int ox, float* c) {
    const float* m = inv + b * 6;
    const float ux = m[0] * ox + m[1] * oy + m[2], uy = m[3] * ox + m[4] * oy + m[5];
    if (!(ux >= -0.5f && ux <= p.w - 0.5f && uy >= -0.5f && uy <= p.h - 0.5f)) {     // NaN lands here too
        c[0] = c[1] = c[2] = 0.f;
        return;
    }
    const float sy = (float)p.hs / p.h, sx = (float)p.ws / p.w;
    float fy = (uy + 0.5f) * sy - 0.5f, fx = (ux + 0.5f) * sx - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    // u up to w-0.5 reaches ws-0.5 in the source: the upper clamp only keeps the gather in bounds (x1 == x0 there, so the
    // weight does not matter and the value is the plain rule's)
    const int y0 = min((int)fy, p.hs - 1), x0 = min((int)fx, p.ws - 1);
    const int y1 = y0 + 1 < p.hs ? y0 + 1 : p.hs - 1, x1 = x0 + 1 < p.ws ? x0 + 1 : p.ws - 1;
    const float wy = fy - y0, wx = fx - x0;
    const unsigned char* base = p.src + (long)b * p.hs * p.ws * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a00 = base[((long)y0 * p.ws + x0) * 3 + ch], a01 = base[((long)y0 * p.ws + x1) * 3 + ch];
        const float a10 = base[((long)y1 * p.ws + x0) * 3 + ch], a11 = base[((long)y1 * p.ws + x1) * 3 + ch];
        const float top = a00 + (a01 - a00) * wx, bot = a10 + (a11 - a10) * wx;
        c[ch] = (top + (bot - top) * wy) * (1.f / 255.f);
    }
}

// One kernel pair for the four pipelines.  WARP and JITTER are compile-time switches: every instantiation contains only its own
// pipeline's code and matches the register / scratch / occupancy table of the hand-written sibling it replaced (tools/kres.py);
// the arguments an instantiation does not use (factors / order / partial without JITTER, inv without WARP) are passed as null
// and never read.
template <bool WARP>
__device__ __forceinline__ void u8_sample(const U8Args& p, const float* inv, int b, int oy, int ox, float* c) {
    if constexpr (WARP) u8_warp_bilinear(p, inv, b, oy, ox, c);
    else u8_bilinear(p, b, oy, ox, c);
}

// with WARP, contrast's grey mean is taken over the WARPED image, black fill included (the reference warps offline, then
// jitters online)
template <bool WARP>
__global__ __launch_bounds__(256) void jitter_mean_kernel(const U8Args p, const float* factors, const int* order, double* partial,
                                                          const float* inv) {
    __shared__ double red[256];
    const int b = blockIdx.y, strip = blockIdx.x;
    const float* f = factors + b * 4;
    const int* ord = order + b * 4;
    int kc = 4;                                         // position of the contrast op (4 = absent)
    for (int k = 3; k >= 0; --k)
        if (ord[k] == 1) kc = k;
    double acc = 0.0;
    const int rows = (p.h + CJ_STRIPS - 1) / CJ_STRIPS;
    const int y0 = strip * rows, y1 = min(p.h, y0 + rows);
    if (kc < 4)
        for (int i = threadIdx.x; i < (y1 - y0) * p.w; i += 256) {
            float c[3];
            u8_sample<WARP>(p, inv, b, y0 + i / p.w, i % p.w, c);
            cj_apply(c, f, ord, 0, kc, 0.f);
            acc += (double)cj_gray(c);
        }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[b * CJ_STRIPS + strip] = red[0];
}

template <typename T, bool WARP, bool JITTER>
__global__ void image_u8_kernel(const U8Args p, const float* factors, const int* order, const double* partial, const float* inv) {
    const long total = (long)p.n * p.hp * p.wp;
    T* dst = (T*)p.dst;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % p.wp);
        const long t = i / p.wp;
        const int y = (int)(t % p.hp), b = (int)(t / p.hp);
        const int oy = y - p.pad, ox = x - p.pad;
        float v[3] = {0.f, 0.f, 0.f};
        if ((unsigned)oy < (unsigned)p.h && (unsigned)ox < (unsigned)p.w) {
            float mean = 0.f;
            if constexpr (JITTER) {
                double m = 0.0;
                for (int k = 0; k < CJ_STRIPS; ++k) m += partial[b * CJ_STRIPS + k];
                mean = (float)(m / ((double)p.h * p.w));
            }
            float c[3];
            u8_sample<WARP>(p, inv, b, oy, ox, c);
            if constexpr (JITTER) cj_apply(c, factors + b * 4, order + b * 4, 0, 4, mean);       // black pixels are jittered too
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = (c[ch] - p.mean[ch]) * p.istd[ch];
        }
        T* o = dst + i * 4;
        o[0] = from_f<T>(v[0]); o[1] = from_f<T>(v[1]); o[2] = from_f<T>(v[2]); o[3] = from_f<T>(0.f);
    }
}

// Checks the arguments the three entries share and fills `a`; returns the apply kernel's grid, 0 when an argument is bad.
static int u8_args(U8Args& a, const unsigned char* hwc, void* out, int n, int hs, int ws, int h, int w, int pad, int wp,
                   const float* mean3, const float* std3) {
    if (!(hwc && out && mean3 && std3 && n > 0 && hs > 0 && ws > 0 && h > 0 && w > 0 && pad >= 0 && wp >= w + 2 * pad)) return 0;
    a.src = hwc; a.dst = out; a.n = n; a.hs = hs; a.ws = ws; a.h = h; a.w = w; a.pad = pad; a.hp = h + 2 * pad; a.wp = wp;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.istd[c] = 1.f / std3[c]; }
    return lh_grid((long)n * a.hp * wp, 8192);
}

// the grey-mean reduction (JITTER only), then the apply kernel; nothing is launched for an unsupported dtype
template <bool WARP, bool JITTER>
static int u8_launch(const U8Args& a, int grid, const float* factors, const int* order, void* workspace, const float* inv, int dtype,
                     void* stream, const char* what) {
    LH_REQUIRE(lh_dtype_size(dtype) > 0, "unsupported dtype %d", dtype);
    if constexpr (JITTER)
        hipLaunchKernelGGL((jitter_mean_kernel<WARP>), dim3(CJ_STRIPS, a.n), dim3(256), 0, (hipStream_t)stream, a, factors, order,
                           (double*)workspace, inv);
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((image_u8_kernel<T, WARP, JITTER>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a,
                                                   factors, order, (const double*)workspace, inv));
    LH_LAUNCH_CHECK(what);
    return LH_OK;
}

extern "C" int lh_image_u8_to_nhwc4(const unsigned char* hwc, void* out, int n, int hs, int ws, int h, int w, int pad, int wp,
                                    const float* mean3, const float* std3, int dtype, void* stream) {
    U8Args a;
    const int grid = u8_args(a, hwc, out, n, hs, ws, h, w, pad, wp, mean3, std3);
    LH_REQUIRE(grid, "lh_image_u8_to_nhwc4: bad arguments");
    return u8_launch<false, false>(a, grid, nullptr, nullptr, nullptr, nullptr, dtype, stream, "image_u8_to_nhwc4 launch");
}

extern "C" size_t lh_image_jitter_workspace_bytes(int n) { return (size_t)n * CJ_STRIPS * sizeof(double); }

extern "C" int lh_image_u8_jitter_to_nhwc4(const unsigned char* hwc, void* out, int n, int hs, int ws, int h, int w, int pad, int wp,
                                           const float* mean3, const float* std3, const float* factors_dev, const int* order_dev,
                                           void* workspace, int dtype, void* stream) {
    U8Args a;
    const int grid = u8_args(a, hwc, out, n, hs, ws, h, w, pad, wp, mean3, std3);
    LH_REQUIRE(grid && factors_dev && order_dev && workspace, "lh_image_u8_jitter_to_nhwc4: bad arguments");
    return u8_launch<false, true>(a, grid, factors_dev, order_dev, workspace, nullptr, dtype, stream, "image_u8_jitter_to_nhwc4 launch");
}

extern "C" int lh_image_u8_warp_to_nhwc4(const unsigned char* hwc, void* out, int n, int hs, int ws, int h, int w, int pad, int wp,
                                         const float* mean3, const float* std3, const float* inv_dev, const float* factors_dev,
                                         const int* order_dev, void* workspace, int dtype, void* stream) {
    U8Args a;
    const int grid = u8_args(a, hwc, out, n, hs, ws, h, w, pad, wp, mean3, std3);
    LH_REQUIRE(grid && inv_dev, "lh_image_u8_warp_to_nhwc4: bad arguments");
    LH_REQUIRE(!factors_dev || (order_dev && workspace), "lh_image_u8_warp_to_nhwc4: ColorJitter needs order_dev and workspace (null)");
    if (!factors_dev)
        return u8_launch<true, false>(a, grid, nullptr, nullptr, nullptr, inv_dev, dtype, stream, "image_u8_warp_to_nhwc4 launch");
    return u8_launch<true, true>(a, grid, factors_dev, order_dev, workspace, inv_dev, dtype, stream, "image_u8_warp_jitter_to_nhwc4 launch");
}

// keypoints through the forward matrix of the warp: p' = (a x + b y + c, d x + e y + f), joints that leave the frame are kept
// (lh_gaussian_target renders them as the reference does: a zero map or a clipped patch)
__global__ void affine_points_kernel(const float* pts, int pstride, const float* fwd, float* out, int ostride, int b, int j) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b * j) return;
    const float* m = fwd + (i / j) * 6;
    const float x = pts[(long)i * pstride], y = pts[(long)i * pstride + 1];
    out[(long)i * ostride] = m[0] * x + m[1] * y + m[2];
    out[(long)i * ostride + 1] = m[3] * x + m[4] * y + m[5];
}

extern "C" int lh_affine_points(const float* pts, int pstride, const float* fwd_dev, float* out, int ostride, int b, int j, void* stream) {
    LH_REQUIRE(pts && fwd_dev && out && pstride >= 2 && ostride >= 2 && b > 0 && j > 0 && (long)b * j < (1L << 31),
               "lh_affine_points: bad arguments");
    hipLaunchKernelGGL(affine_points_kernel, dim3((b * j + 255) / 256), dim3(256), 0, (hipStream_t)stream, pts, pstride, fwd_dev, out, ostride,
                       b, j);
    LH_LAUNCH_CHECK("affine_points launch");
    return LH_OK;
}

// Flip test (TEST.FLIP_TEST of the reference's configs): the second forward of a flip-test step reads the stem's padded NHWC4
// image mirrored in place, img'[y][x] = img[y][w-1-x] over the w interior pixels of every row.  The padding is not touched, so
// the zero border stays where the stem expects it.  The launch takes the place of the image launch in that pass: one kernel
// serves every input path (float, uint8, ColorJitter, warp), and what the stem reads is bit for bit the mirror of what the
// first pass fed it.  A pixel record (4 channels) moves as one word R: 8 bytes for 16-bit dtypes, 16 for fp32.  Thread k of
// a row swaps records k and w-1-k, so consecutive lanes read and write consecutive records on both sides of the row.
template <typename R>
__global__ void nhwc4_mirror_kernel(R* img, int h, int w, int pad, int hp, int wp, unsigned half, unsigned total) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / half;                          // interior row b * h + y
        const int k = (int)(i - r * half);
        const unsigned b = r / (unsigned)h, y = r - b * (unsigned)h;
        R* row = img + ((long)(b * (unsigned)hp + y + (unsigned)pad) * wp + pad);
        const R lo = row[k], hi = row[w - 1 - k];
        row[k] = hi;
        row[w - 1 - k] = lo;
    }
}

extern "C" int lh_nhwc4_mirror(void* img, int n, int h, int w, int pad, int wp, int dtype, void* stream) {
    LH_REQUIRE(img && n > 0 && h > 0 && w > 0 && pad >= 0 && wp >= w + 2 * pad, "lh_nhwc4_mirror: bad arguments");
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0, "lh_nhwc4_mirror: unsupported dtype %d", dtype);
    const int hp = h + 2 * pad;
    LH_REQUIRE((long)n * hp * wp < (1L << 31), "lh_nhwc4_mirror: image batch too large for 32-bit pixel indices");
    const unsigned half = (unsigned)(w / 2), total = (unsigned)n * (unsigned)h * half;
    if (total == 0) return LH_OK;                             // w == 1: the mirror is the identity
    const int grid = lh_grid(total, 8192);
    if (es == 2)
        hipLaunchKernelGGL((nhwc4_mirror_kernel<uint2>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (uint2*)img, h, w, pad, hp, wp,
                           half, total);
    else
        hipLaunchKernelGGL((nhwc4_mirror_kernel<uint4>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (uint4*)img, h, w, pad, hp, wp,
                           half, total);
    LH_LAUNCH_CHECK("nhwc4_mirror launch");
    return LH_OK;
}

template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* src, float* dst, int n, int hw, int c, int cs, int vec) {
    const long total = (long)n * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw), p = (int)(i % hw);
        const T* s = src + i * cs;
        constexpr int EPC = 16 / sizeof(T);
        if (vec) {                               // whole, 16-byte ALIGNED chunks per pixel: one vector load per EPC channels (was one 2-byte load per channel)
            for (int c0 = 0; c0 < c; c0 += EPC) {
                float v[EPC];
                unpack16<T>(*reinterpret_cast<const uint4*>(s + c0), v);
#pragma unroll
                for (int e = 0; e < EPC; ++e)
                    if (c0 + e < c) dst[((long)b * c + c0 + e) * hw + p] = v[e];
            }
        } else {
            for (int ch = 0; ch < c; ++ch) dst[((long)b * c + ch) * hw + p] = to_f<T>(s[ch]);
        }
    }
}
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* src, T* dst, int n, int hw, int c, int cs, int vec) {
    const long total = (long)n * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw), p = (int)(i % hw);
        T* d = dst + i * cs;
        constexpr int EPC = 16 / sizeof(T);
        if (vec) {                               // whole, 16-byte aligned chunks per pixel: gather EPC channels, one vector store
            for (int c0 = 0; c0 < cs; c0 += EPC) {
                float v[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) v[e] = c0 + e < c ? src[((long)b * c + c0 + e) * hw + p] : 0.f;
                *reinterpret_cast<uint4*>(d + c0) = pack16<T>(v);
            }
        } else {
            for (int ch = 0; ch < cs; ++ch) d[ch] = from_f<T>(ch < c ? src[((long)b * c + ch) * hw + p] : 0.f);
        }
    }
}

extern "C" int lh_nhwc_to_nchw_f32(const void* nhwc, float* nchw, int n, int h, int w, int c, int c_stride, int dtype,
                                   void* stream) {
    LH_REQUIRE(nhwc && nchw && n > 0 && h > 0 && w > 0 && c > 0 && c_stride >= c, "lh_nhwc_to_nchw_f32: bad arguments");
    const long total = (long)n * h * w;
    const int grid = lh_grid(total, 8192);
    // the vector path needs 16-byte aligned pixel rows: a channel-sliced base pointer (base + 4 channels, stride 64) takes the scalar loop
    const int es = lh_dtype_size(dtype);
    const int vec = es > 0 && c_stride % (16 / es) == 0 && ((uintptr_t)nhwc & 15) == 0;
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((nhwc_to_nchw_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream,
                                                   (const T*)nhwc, nchw, n, h * w, c, c_stride, vec));
    LH_LAUNCH_CHECK("nhwc_to_nchw launch");
    return LH_OK;
}
extern "C" int lh_nchw_f32_to_nhwc(const float* nchw, void* nhwc, int n, int h, int w, int c, int c_stride, int dtype,
                                   void* stream) {
    LH_REQUIRE(nhwc && nchw && n > 0 && h > 0 && w > 0 && c > 0 && c_stride >= c, "lh_nchw_f32_to_nhwc: bad arguments");
    const long total = (long)n * h * w;
    const int grid = lh_grid(total, 8192);
    const int es = lh_dtype_size(dtype);
    const int vec = es > 0 && c_stride % (16 / es) == 0 && ((uintptr_t)nhwc & 15) == 0;
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((nchw_to_nhwc_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream,
                                                   nchw, (T*)nhwc, n, h * w, c, c_stride, vec));
    LH_LAUNCH_CHECK("nchw_to_nhwc launch");
    return LH_OK;
}
