// Error channel and version, bias-gradient channel sums, strided fp32 copy, collective staging (bf16 cast, chunk sum).
#include "common.h"
#include <stdarg.h>
#include <stdio.h>

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
void lh_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* lh_last_error(void) { return g_err; }
extern "C" int lh_version(void) { return 100; }
extern "C" int lh_dtype_size(int dtype) {
    switch (dtype) {
        case LH_F32: return 4;
        case LH_BF16: return 2;
        case LH_F16: return 2;
        default: return 0;
    }
}

// ------------------------------------------------------------------------------------------------ head bias gradient
// d(bias)[c] = sum over n, h, w of an NCHW fp32 gradient (the head's 1x1 convolution with bias, pose_resnet.py:169-175):
// one workgroup per (channel, slice of the batch), fp64 partials, fixed order -> deterministic.
__global__ __launch_bounds__(256) void channel_sum_nchw_kernel(const float* x, int n, int c, int hw, double* partial, int slices) {
    __shared__ double red[4];
    const int ch = blockIdx.x, sl = blockIdx.y;
    const int n0 = (int)((long)n * sl / slices), n1 = (int)((long)n * (sl + 1) / slices);
    double acc = 0.0;
    for (int b = n0; b < n1; ++b) {
        const float* p = x + ((long)b * c + ch) * hw;
        if ((hw & 3) == 0) {                     // planes are 16-byte aligned: four elements per load, same summation order per thread
            const float4* p4 = reinterpret_cast<const float4*>(p);
            for (int i = threadIdx.x; i < hw / 4; i += 256) {
                const float4 v = p4[i];
                acc += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
            }
        } else {
            for (int i = threadIdx.x; i < hw; i += 256) acc += (double)p[i];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long)ch * slices + sl] = red[0] + red[1] + red[2] + red[3];
}

__global__ void channel_sum_final_kernel(const double* partial, int c, int slices, float* out) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    double a = 0.0;
    for (int s = 0; s < slices; ++s) a += partial[(long)ch * slices + s];
    out[ch] = (float)a;
}

extern "C" size_t lh_channel_sum_workspace_bytes(int c) { return (size_t)c * 64 * sizeof(double); }

extern "C" int lh_channel_sum_nchw(const float* x, int n, int c, int hw, float* out, void* workspace, void* stream) {
    LH_REQUIRE(x && out && workspace && n > 0 && c > 0 && hw > 0, "lh_channel_sum_nchw: bad arguments");
    const int slices = n < 64 ? n : 64;
    hipLaunchKernelGGL(channel_sum_nchw_kernel, dim3(c, slices), dim3(256), 0, (hipStream_t)stream, x, n, c, hw, (double*)workspace, slices);
    hipLaunchKernelGGL(channel_sum_final_kernel, dim3((c + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, c, slices, out);
    LH_LAUNCH_CHECK("channel_sum launch");
    return LH_OK;
}

// Bias gradient of a convolution / transposed convolution with bias inside the network (DECONV_WITH_BIAS,
// pose_resnet.py:149,227): out[ch] = sum over the pixels of an NHWC gradient of the run precision, channels [0, c) of rows of
// `stride` elements.  A workgroup takes a slice of the pixels: thread (row group r, 16-byte chunk q) sums its chunk's
// elements over rows r, r + R, ... in fp64, the row groups are folded through LDS in a fixed order, and the slices by
// channel_sum_final_kernel: deterministic.
template <typename T>
__global__ __launch_bounds__(256) void channel_sum_nhwc_kernel(const T* x, long pixels, int c, int stride, double* partial, int slices) {
    constexpr int EPC = 16 / sizeof(T);
    __shared__ double red[256 * EPC];
    const int nchunk = (c + EPC - 1) / EPC;              // 16-byte chunks per row that hold requested channels
    const int sl = blockIdx.x;
    const long p0 = pixels * sl / slices, p1 = pixels * (sl + 1) / slices;
    for (int q0 = 0; q0 < nchunk; q0 += 256) {           // <= 256 chunks at a time (2048 bf16 channels)
        const int cw = nchunk - q0 < 256 ? nchunk - q0 : 256;
        int R = 1;                                       // row groups: the largest power of two with R * cw <= 256
        while (R * 2 * cw <= 256) R *= 2;
        const int r = threadIdx.x / cw, q = threadIdx.x - r * cw;
        double acc[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.0;
        if (r < R) {
            for (long px = p0 + r; px < p1; px += R) {
                float v[EPC];
                unpack16<T>(*reinterpret_cast<const uint4*>(x + px * stride + (long)(q0 + q) * EPC), v);
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] += (double)v[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[threadIdx.x * EPC + e] = acc[e];
        __syncthreads();
        for (int t = threadIdx.x; t < cw * EPC; t += 256) {
            const int qq = t / EPC, e = t - qq * EPC, ch = (q0 + qq) * EPC + e;
            double a = 0.0;
            for (int rr = 0; rr < R; ++rr) a += red[(rr * cw + qq) * EPC + e];
            if (ch < c) partial[(long)ch * slices + sl] = a;
        }
    }
}

extern "C" int lh_channel_sum_nhwc(const void* x, long pixels, int c, int pix_stride, float* out, void* workspace, int dtype, void* stream) {
    LH_REQUIRE(x && out && workspace && pixels > 0 && c > 0 && pix_stride >= c, "lh_channel_sum_nhwc: bad arguments");
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0 && (pix_stride * es) % 16 == 0, "lh_channel_sum_nhwc: pixel rows must be 16-byte aligned (stride %d, dtype %d)", pix_stride, dtype);
    const int slices = pixels < 64 ? (int)pixels : 64;
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((channel_sum_nhwc_kernel<T>), dim3(slices), dim3(256), 0, (hipStream_t)stream,
                                                   (const T*)x, pixels, c, pix_stride, (double*)workspace, slices));
    hipLaunchKernelGGL(channel_sum_final_kernel, dim3((c + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, c, slices, out);
    LH_LAUNCH_CHECK("channel_sum_nhwc launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ strided fp32 copy
// dst[i0][i1][i2][i3] = src[i0][i1][i2][i3] with arbitrary element strides on both sides: the small layout shuffles of a
// step (stem weight [O][3][k][k] <-> [O][k][k'][4] staging, head-gradient crop, bias padding) without a framework op.
__global__ void copy_strided_f32_kernel(float* dst, const float* src, int n0, int n1, int n2, int n3, long d0, long d1, long d2,
                                        long d3, long s0, long s1, long s2, long s3) {
    const long total = (long)n0 * n1 * n2 * n3;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int i3 = (int)(i % n3);
        long t = i / n3;
        const int i2 = (int)(t % n2);
        t /= n2;
        const int i1 = (int)(t % n1), i0 = (int)(t / n1);
        dst[i0 * d0 + i1 * d1 + i2 * d2 + i3 * d3] = src[i0 * s0 + i1 * s1 + i2 * s2 + i3 * s3];
    }
}

extern "C" int lh_copy_strided_f32(float* dst, const float* src, const int* shape4, const long* dst_strides4, const long* src_strides4,
                                   void* stream) {
    LH_REQUIRE(dst && src && shape4 && dst_strides4 && src_strides4, "lh_copy_strided_f32: null pointer");
    const long total = (long)shape4[0] * shape4[1] * shape4[2] * shape4[3];
    LH_REQUIRE(shape4[0] > 0 && shape4[1] > 0 && shape4[2] > 0 && shape4[3] > 0, "lh_copy_strided_f32: empty shape");
    const int grid = lh_grid(total, 1024);
    hipLaunchKernelGGL(copy_strided_f32_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dst, src, shape4[0], shape4[1], shape4[2],
                       shape4[3], dst_strides4[0], dst_strides4[1], dst_strides4[2], dst_strides4[3], src_strides4[0], src_strides4[1],
                       src_strides4[2], src_strides4[3]);
    LH_LAUNCH_CHECK("copy_strided_f32 launch");
    return LH_OK;
}

// ---- gradient bucket staging for bf16 collectives (parallel.GradSync(compress="bf16")): fp32 arena slice <-> bf16 buffer,
// 16 bytes of bf16 per lane (round to nearest even through the hardware convert; NaN stays NaN)
__global__ void cast_f32_bf16_kernel(const float* __restrict__ src, bf16* __restrict__ dst, long n) {
    const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    const long stride = (long)gridDim.x * blockDim.x * 8;
    for (long i = i0; i < n; i += stride) {
        if (i + 8 <= n && (((size_t)(src + i) | (size_t)(dst + i)) & 15) == 0) {
            const float4 a = *reinterpret_cast<const float4*>(src + i), b = *reinterpret_cast<const float4*>(src + i + 4);
            Vec16<bf16> v;
            v.e[0] = (bf16)a.x; v.e[1] = (bf16)a.y; v.e[2] = (bf16)a.z; v.e[3] = (bf16)a.w;
            v.e[4] = (bf16)b.x; v.e[5] = (bf16)b.y; v.e[6] = (bf16)b.z; v.e[7] = (bf16)b.w;
            *reinterpret_cast<uint4*>(dst + i) = v.u;
        } else {
            for (long k = i; k < n && k < i + 8; ++k) dst[k] = (bf16)src[k];
        }
    }
}

__global__ void cast_bf16_f32_kernel(const bf16* __restrict__ src, float* __restrict__ dst, long n) {
    const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    const long stride = (long)gridDim.x * blockDim.x * 8;
    for (long i = i0; i < n; i += stride) {
        if (i + 8 <= n && (((size_t)(src + i) | (size_t)(dst + i)) & 15) == 0) {
            Vec16<bf16> v;
            v.u = *reinterpret_cast<const uint4*>(src + i);
            *reinterpret_cast<float4*>(dst + i) = float4{(float)v.e[0], (float)v.e[1], (float)v.e[2], (float)v.e[3]};
            *reinterpret_cast<float4*>(dst + i + 4) = float4{(float)v.e[4], (float)v.e[5], (float)v.e[6], (float)v.e[7]};
        } else {
            for (long k = i; k < n && k < i + 8; ++k) dst[k] = (float)src[k];
        }
    }
}

extern "C" int lh_cast_f32_bf16(float* src, void* dst, long n, int to_f32, void* stream) {
    LH_REQUIRE(src && dst && n > 0, "lh_cast_f32_bf16: bad arguments");
    const long groups = (n + 7) / 8;
    const int grid = lh_grid(groups, 8192);
    if (to_f32) hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)dst, src, n);
    else hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, n);
    LH_LAUNCH_CHECK("cast_f32_bf16 launch");
    return LH_OK;
}

// The local half of the DIRECT gradient exchange (parallel.GradSync(algo="direct"); SURVEY 8e: reduce-scatter + all-gather with all
// seven xGMI peers at once instead of a ring): after the all-to-all a rank holds `rows` chunks of `len` elements -- chunk r = rank r's
// contribution to the slice this rank owns -- and sums them IN RANK ORDER (fp32 accumulation; bf16 chunks are widened, the sum is
// rounded once), so every rank's owned slice, and after the all-gather every rank's whole bucket, holds bit-identical values.
template <typename T>
__global__ void sum_chunks_kernel(const T* __restrict__ in, T* __restrict__ out, int rows, long len) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
        float acc = (float)in[i];
        for (int r = 1; r < rows; ++r) acc += (float)in[(long)r * len + i];
        out[i] = (T)acc;
    }
}

extern "C" int lh_sum_chunks(const void* in, void* out, int rows, long len, int dtype, void* stream) {
    LH_REQUIRE(in && out && rows >= 1 && len > 0, "lh_sum_chunks: bad arguments");
    LH_REQUIRE(dtype == LH_F32 || dtype == LH_BF16, "lh_sum_chunks: fp32 or bf16 chunks (dtype %d)", dtype);
    const int grid = lh_grid(len, 4096);
    if (dtype == LH_F32) hipLaunchKernelGGL(sum_chunks_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)in, (float*)out, rows, len);
    else hipLaunchKernelGGL(sum_chunks_kernel<bf16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16*)in, (bf16*)out, rows, len);
    LH_LAUNCH_CHECK("sum_chunks launch");
    return LH_OK;
}
