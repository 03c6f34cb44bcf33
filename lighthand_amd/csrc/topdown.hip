// Top-down inference on full frames: hand box -> crop matrix, crop of a shared uint8 frame buffer to padded NHWC4, keypoints -> next box.
// Coordinates are pixel indices (pixel centres on the integers, an image spans [-0.5, size-0.5]); a box is (x0, y0, x1, y1) in them.
// All arithmetic is fp32 in the order written (-ffp-contract=off): lighthand_amd/topdown.py restates it in numpy.
#include "common.h"
#include "color_jitter.h"

// ------------------------------------------------------------------------------------------------ box -> matrix
// mat[i] takes a CROP pixel index to a FRAME pixel index: the crop kernel samples through it and lh_affine_points moves the decoded
// keypoints back to the frame through it -- one matrix per slot, no inverse.  The padded box keeps the crop's aspect ratio.
__global__ void box_affine_kernel(const float* boxes, const int* frame_index, int b, int n_frames, float h, float w, float padding,
                                  float* mat, int* src_frame) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b) return;
    const float x0 = boxes[i * 4], y0 = boxes[i * 4 + 1], x1 = boxes[i * 4 + 2], y1 = boxes[i * 4 + 3];
    const int fi = frame_index[i];
    const float bw = x1 - x0, bh = y1 - y0;
    const bool ok = fi >= 0 && fi < n_frames && isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && bw > 0.f && bh > 0.f;
    float* m = mat + i * 6;
    if (!ok) {                                                    // an empty slot: black crop, keypoints at (0, 0)
        src_frame[i] = -1;
        m[0] = m[1] = m[2] = m[3] = m[4] = m[5] = 0.f;
        return;
    }
    const float cx = (x0 + x1) * 0.5f, cy = (y0 + y1) * 0.5f;
    const float sw = padding * fmaxf(bw, bh * w / h), sh = sw * h / w, a = sw / w;
    src_frame[i] = fi;
    m[0] = a;   m[1] = 0.f; m[2] = (cx - sw * 0.5f) + a * 0.5f;
    m[3] = 0.f; m[4] = a;   m[5] = (cy - sh * 0.5f) + a * 0.5f;
}

extern "C" int lh_box_affine(const float* boxes_dev, const int* frame_index_dev, int b, int n_frames, int h, int w, float padding,
                             float* mat_dev, int* src_frame_dev, void* stream) {
    LH_REQUIRE(boxes_dev && frame_index_dev && mat_dev && src_frame_dev && b > 0 && n_frames > 0 && h > 0 && w > 0 && padding > 0.f
               && padding <= 3.0e38f, "lh_box_affine: bad arguments");
    hipLaunchKernelGGL(box_affine_kernel, dim3((b + 63) / 64), dim3(64), 0, (hipStream_t)stream, boxes_dev, frame_index_dev, b, n_frames,
                       (float)h, (float)w, padding, mat_dev, src_frame_dev);
    LH_LAUNCH_CHECK("box_affine launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ frames -> crops
// Slot blockIdx.y reads frame src_frame[slot] of a buffer every slot shares: several boxes per frame, frames of any size.  The slot's
// matrix and frame number are the same for the whole workgroup (scalar loads); one thread per pixel of the padded output, as
// image_u8_kernel.  A gather over bytes: neighbouring lanes read neighbouring source pixels (a box maps rows to rows), the four taps
// of a pixel share cache lines with its neighbours', and the frame's reuse across the boxes that read it is the L2's.
//
// Area sampling of minified ROIs (lh_frames_crop_area_to_nhwc4; max_taps = 1 is the plain crop).  One bilinear sample per crop pixel
// skips frame pixels as soon as a crop pixel covers more than one of them, so a minified crop averages kx x ky samples spread evenly
// over each crop pixel's footprint instead.  The rule, fp32 in this order; topdown.py's frames_crop_host / crop_taps_host restate it.
// Per slot, from its matrix:
//     sx = sqrtf(m0*m0 + m3*m3), sy = sqrtf(m1*m1 + m4*m4)          frame pixels per crop pixel along the crop's x and y axes
//     kx = sx > 1.015625f && isfinite(sx) ? min(max_taps, (int)ceilf(fminf(sx, 64.f))) : 1, ky likewise from sy
// A NaN scale fails the comparison and gives 1, an infinite one is given 1 (such a matrix puts every sample outside the frame); the
// 1/64 slack keeps a ROI at scale 1 + rounding error on the single-sample path.
// Per output pixel (ox, oy), j = 0..ky-1 outside and i = 0..kx-1 inside:
//     dy = (float)(2*j + 1 - ky) / (float)(2*ky), uy = (float)oy + dy;  dx, ux likewise from i, kx and ox
//     (the offset (j + 0.5) / ky - 0.5 rounded ONCE: formed as (j + 0.5f) / ky - 0.5f it is -0.33333331 for ky = 3, and the first
//     sample of an aligned s = 3 crop then lands 6e-8 beside its pixel instead of on it)
//     fx = (m0*ux + m1*uy) + m2, fy = (m3*ux + m4*uy) + m5
//     acc[ch] += the plain crop's sample at (fx, fy) on the raw 0..255 values: the same inside test, edge clamp and blend
//                top + (bot - top) * wy; a sample outside the frame (or a NaN) adds 0
// then c[ch] = (acc[ch] * (1.f / (float)(kx*ky))) * (1.f / 255.f), Normalize and the store as in the plain crop.
// With kx = ky = 1 the offsets are 0 and acc * 1.f = acc: the plain crop bit for bit (the kernel takes the plain body then).  A pixel
// whose samples all fall outside is exactly black.  An aligned integer minification s <= max_taps (m = (s, 0, (s-1)/2, 0, s, (s-1)/2))
// puts the samples on the integer pixels s*ox + i for s = 2, 3, 4, 5, 6, 8 and crops up to 512 pixels a side (s = 7 does not:
// 3/7 has no short binary form): the exact mean of the s x s block.  Above max_taps the taps are more than one frame
// pixel apart, so aliasing is reduced, not removed.  kx and ky are the same for the whole workgroup (the slot is blockIdx.y): the
// tap loops are uniform, no divergence.  Texels are byte loads as in the plain crop: the taps of a pixel and of its neighbours share
// cache lines, and the frame's reuse is the L2's.  Which pixel a thread takes does not enter the rule: a slot whose crop rows run
// across the frame's rows is walked in 8 x 8 tiles (crop_pixels).
//
// NV12 frames (lh_frames_crop_yuv_to_nhwc4): the same kernel, format is a workgroup-uniform switch in front of the pixel loops, so the
// RGB entries run the bodies they always ran.  Frame f starts at byte f * frame_stride; luma byte (x, y) is at y*pitch + x, Cb and Cr of
// chroma sample (cx, cy) at uv_offset + cy*pitch + 2*cx and + 1; wc = ws/2, hc = hs/2.  Every sample at (fx, fy) -- the pixel's centre
// or one tap of the area rule -- passes the RGB inside test and lower clamp (cx_, cy_), then, fp32 in this order:
//     Y    = the RGB sample of one channel on the luma plane: same indices, upper index clamp, weights and blend
//     gx   = siting == 0 ? cx_ * 0.5f : (cx_ - 0.5f) * 0.5f, gy = (cy_ - 0.5f) * 0.5f       (0: chroma co-sited with even luma
//            columns, 1: centred between them; vertically always centred)
//     gx   = fminf(fmaxf(gx, 0), wc-1), gy = fminf(fmaxf(gy, 0), hc-1)
//     U, V = the same blend on the chroma plane at (gx, gy): x0 = min((int)gx, wc-1), x1 = min(x0+1, wc-1), y likewise
//     e    = (Y - o[0], U - o[1], V - o[2]),  s[c] = fminf(fmaxf((k[c][0]*e0 + k[c][1]*e1) + k[c][2]*e2, 0.f), 255.f)
// and s is the RGB path's sample from there on (* 1/255 or the tap sum, Normalize, store).  topdown.py: frames_crop_nv12_host.
// A sample reads 4 luma and 8 chroma bytes; the highest one is uv_offset + (hc-1)*pitch + ws - 1 < frame_stride (checked on the host).
//
// ColorJitter on the crop (lh_frames_crop_jitter_to_nhwc4, training on frames): the uint8 input kernels' rule (color_jitter.h) on the
// pixel's c[3] in 0..1 -- after the single sample, the tap average or the YUV conversion -- in the slot's op order, before Normalize.
// Two launches of this kernel.  The grey-mean mode (op = LH_CROP_GREY_MEAN, the fp32 instantiation whatever the crop's dtype: the
// samples are fp32 in all three) walks the slot's interior through the crop's own sample path (the same kx, ky, the same walk),
// applies the ops that precede contrast and reduces cj_gray in fp64: per thread in walk order, then a fixed tree in LDS, one partial
// per workgroup into workspace[slot][CJ_STRIPS] (grid (CJ_STRIPS, b), no atomics: a replay is bit-reproducible).  Pixels that fell
// outside the frame are black and count, as the warped uint8 path counts its black fill.  A slot without a contrast op writes zeros
// and samples nothing.  The apply mode (op = LH_CROP with jfactors != null, a workgroup-uniform switch in front of the pixel loops as
// format is; also the fp32 instantiation's, which then stores in jdtype: the 16-bit instantiations carry no jitter code at all) sums
// the slot's partials in index order once per workgroup, mean = (float)(sum / (h*w)), and runs cj_apply(c, factors, order, 0, 4, mean)
// between the sample and Normalize.  Order (-1, -1, -1, -1) touches nothing: the un-jittered crop bit for bit.  An empty slot stays
// black: every op maps black with mean 0 to black.  topdown.py: frames_crop_jitter_host.
//
// Decoder surfaces and the other 4:2:0 flavours (lh_frames_crop_surfaces_to_nhwc4): where a sample's bytes are.  The frame source is the
// buffer above (frame f at byte f * frame_stride) or a SURFACE TABLE, int64 [n_frames] in device memory: entry f is the device address
// of frame f, read at every launch -- the surfaces of a captured graph change with no recapture.  The entry is a scalar load (the slot
// is blockIdx.y) and is tested before any address is formed from it: 0 is an empty frame, the slot's crop is black as an empty slot's.
// One plane descriptor (format = LH_FRAMES_420, or LH_FRAMES_420W for 16-bit samples) covers NV12, NV21, planar yuv420p and 10-bit
// P010: luma sample (x, y) at y*pitch + x*sample_bytes, Cb / Cr of chroma sample (cx, cy) at cb_offset / cr_offset + cy*c_pitch +
// cx*c_step.  A 16-bit sample is little-endian and its texel value is (float)(u16 >> 6) * 0.25f -- the 10 significant bits on the
// 8-bit scale, exact in fp32, the low 6 bits never data.  Everything after the texel fetch is the NV12 rule above, in the same order
// (crop_sample_420 is crop_sample_nv12 with the descriptor's addresses), so NV12 through the descriptor gives
// lh_frames_crop_yuv_to_nhwc4's bits.  The sample width picks the body in front of the pixel loops, as format does.
// All of it is the fp32 instantiation's (gen != 0), which then stores in jdtype as the ColorJitter apply mode does: the 16-bit
// instantiations carry none of it.  topdown.py: frames_crop_yuv420_host.
enum { LH_FRAMES_RGB = 0, LH_FRAMES_NV12 = 1, LH_FRAMES_420 = 2, LH_FRAMES_420W = 3 };

struct CropArgs {
    const unsigned char* src;
    void* dst;
    const float* mat;
    const int* src_frame;
    int n_frames, hs, ws, h, w, pad, hp, wp;
    float mean[3], istd[3];
    int max_taps;
    int format, pitch, uv_offset, siting;                         // NV12 only from here (format = LH_FRAMES_RGB: not read)
    long frame_stride;
    float k[9], o[3];
    // The two small entries of training on frames run as modes of this kernel's fp32 instantiation (op != LH_CROP; the resource tables
    // the tests hold the library to admit no new kernel symbol).  op is workgroup-uniform and tested once, in front of everything the
    // crop does; the crop entries pass LH_CROP and read none of the fields below.
    int op, n, j, pstride, ostride;
    const float *in0, *in1, *in2;                                 // perturb: boxes, rot, aug          inverse: points, matrices, -
    const int* iin;                                               //          mirror                            src_frame
    float *out0, *out1;                                           //          boxes', rot'                      points', -
    int* iout;                                                    //          mirror'                           -
    // ColorJitter (the header comment): null = none, and the crop entries without it read none of the three
    const float* jfactors;                                        // [b][4] brightness, contrast, saturation, hue
    const int* jorder;                                            // [b][4] op ids, negative = skip
    double* jpartial;                                             // [b][CJ_STRIPS]: written by LH_CROP_GREY_MEAN, read by the apply mode
    int jdtype;                                                   // the apply mode: the dtype of dst (the launch is the fp32 instantiation's)
    // lh_frames_crop_surfaces_to_nhwc4 (the header comment; gen = 0: none of it is read).  The fp32 instantiation's, stores in jdtype.
    int gen;
    const long long* table;                                       // [n_frames] device addresses (0 = empty), or null: src + f * frame_stride
    int dsc[4];                                                   // LH_FRAMES_420 / 420W: c_pitch, cb_offset, cr_offset, c_step (with pitch, siting)
};
enum { LH_CROP = 0, LH_CROP_ROI_PERTURB = 1, LH_CROP_POINTS_INV = 2, LH_CROP_GREY_MEAN = 3 };
enum { LH_JIT_NONE = 0, LH_JIT_APPLY = 1, LH_JIT_MEAN = 2, LH_JIT_STORE = 3 };      // STORE: no jitter, the store is jit.dtype's

// What a jittered launch carries into the pixel loops: the slot's factors and order, then the grey mean (LH_JIT_APPLY) or the number
// of ops in front of contrast (LH_JIT_MEAN).
struct CropJit {
    const float* f;
    const int* order;
    float mean;
    int kc;
    int dtype;                                                    // LH_JIT_APPLY: what dst holds
};

// One pixel of padded NHWC4, channel 3 = 0.
template <typename T>
__device__ __forceinline__ void crop_store(T* dst, int i, const float v[3]) {
    if constexpr (sizeof(T) == 2) {                               // one 8-byte store per pixel
        union { uint2 u; T e[4]; } pk;
        pk.e[0] = from_f<T>(v[0]); pk.e[1] = from_f<T>(v[1]); pk.e[2] = from_f<T>(v[2]); pk.e[3] = from_f<T>(0.f);
        *reinterpret_cast<uint2*>(dst + (long)i * 4) = pk.u;
    } else {
        T* o = dst + (long)i * 4;
        o[0] = from_f<T>(v[0]); o[1] = from_f<T>(v[1]); o[2] = from_f<T>(v[2]); o[3] = from_f<T>(0.f);
    }
}

// One bilinear sample of the frame at (fx, fy) on the raw 0..255 values; false (s untouched) outside the frame or for a NaN.
__device__ __forceinline__ bool crop_sample(const unsigned char* base, int hs, int ws, float fx, float fy, float s[3]) {
    if (!(fx >= -0.5f && fx <= ws - 0.5f && fy >= -0.5f && fy <= hs - 0.5f)) return false;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    // f up to size-0.5: the upper clamp only keeps the gather in bounds (x1 == x0 there, the weight does not matter)
    const int y0 = min((int)fy, hs - 1), x0 = min((int)fx, ws - 1);
    const int y1 = y0 + 1 < hs ? y0 + 1 : hs - 1, x1 = x0 + 1 < ws ? x0 + 1 : ws - 1;
    const float wy = fy - y0, wx = fx - x0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a00 = base[((long)y0 * ws + x0) * 3 + ch], a01 = base[((long)y0 * ws + x1) * 3 + ch];
        const float a10 = base[((long)y1 * ws + x0) * 3 + ch], a11 = base[((long)y1 * ws + x1) * 3 + ch];
        const float top = a00 + (a01 - a00) * wx, bot = a10 + (a11 - a10) * wx;
        s[ch] = top + (bot - top) * wy;
    }
    return true;
}

// The NV12 sibling (the rule: above): base is the frame's first luma byte.  One frame's bytes are a 32-bit quantity (frame_stride < 2^31).
// csc = k[9], o[3] in VECTOR registers (frames_crop_kernel).
__device__ __forceinline__ bool crop_sample_nv12(const CropArgs& p, const float* csc, const unsigned char* base, float fx, float fy,
                                                 float s[3]) {
    const int hs = p.hs, ws = p.ws, pitch = p.pitch;
    if (!(fx >= -0.5f && fx <= ws - 0.5f && fy >= -0.5f && fy <= hs - 0.5f)) return false;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    float yuv[3];
    {
        const int y0 = min((int)fy, hs - 1), x0 = min((int)fx, ws - 1);
        const int y1 = y0 + 1 < hs ? y0 + 1 : hs - 1, x1 = x0 + 1 < ws ? x0 + 1 : ws - 1;
        const float wy = fy - y0, wx = fx - x0;
        const float a00 = base[y0 * pitch + x0], a01 = base[y0 * pitch + x1];
        const float a10 = base[y1 * pitch + x0], a11 = base[y1 * pitch + x1];
        const float top = a00 + (a01 - a00) * wx, bot = a10 + (a11 - a10) * wx;
        yuv[0] = top + (bot - top) * wy;
    }
    const int hc = hs >> 1, wc = ws >> 1;
    float gx = p.siting == 0 ? fx * 0.5f : (fx - 0.5f) * 0.5f, gy = (fy - 0.5f) * 0.5f;
    gx = fminf(fmaxf(gx, 0.f), (float)(wc - 1));
    gy = fminf(fmaxf(gy, 0.f), (float)(hc - 1));
    const int y0 = min((int)gy, hc - 1), x0 = min((int)gx, wc - 1);
    const int y1 = min(y0 + 1, hc - 1), x1 = min(x0 + 1, wc - 1);
    const float wy = gy - y0, wx = gx - x0;
    const unsigned char* uv = base + p.uv_offset;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const float a00 = uv[y0 * pitch + 2 * x0 + ch], a01 = uv[y0 * pitch + 2 * x1 + ch];
        const float a10 = uv[y1 * pitch + 2 * x0 + ch], a11 = uv[y1 * pitch + 2 * x1 + ch];
        const float top = a00 + (a01 - a00) * wx, bot = a10 + (a11 - a10) * wx;
        yuv[1 + ch] = top + (bot - top) * wy;
    }
    const float e0 = yuv[0] - csc[9], e1 = yuv[1] - csc[10], e2 = yuv[2] - csc[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = fminf(fmaxf((csc[c * 3] * e0 + csc[c * 3 + 1] * e1) + csc[c * 3 + 2] * e2, 0.f), 255.f);
    return true;
}

// The descriptor's sibling (LH_FRAMES_420 / 420W; the header comment): crop_sample_nv12's operations in its order, the texels through
// the plane descriptor.  U = unsigned char: 8-bit samples; unsigned short: P010's.  Offsets are 32-bit (a frame is below 2^31 bytes).
// csc[12..15] hold the bits of c_pitch, cb_offset, cr_offset, c_step: in VECTOR registers like the coefficients in front of them
// (crop_slot) -- as scalars they are more than the kernel has, and the compiler spills scalars to scratch.
template <typename U>
__device__ __forceinline__ float crop_texel(const unsigned char* plane, int off) {
    if constexpr (sizeof(U) == 2) return (float)(*reinterpret_cast<const unsigned short*>(plane + off) >> 6) * 0.25f;
    else return (float)plane[off];
}

template <typename U>
__device__ __forceinline__ bool crop_sample_420(const CropArgs& p, const float* csc, const unsigned char* base, float fx, float fy,
                                                float s[3]) {
    constexpr int SH = sizeof(U) == 2 ? 1 : 0;
    const int hs = p.hs, ws = p.ws, pitch = p.pitch;
    if (!(fx >= -0.5f && fx <= ws - 0.5f && fy >= -0.5f && fy <= hs - 0.5f)) return false;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    float yuv[3];
    {
        const int y0 = min((int)fy, hs - 1), x0 = min((int)fx, ws - 1);
        const int y1 = y0 + 1 < hs ? y0 + 1 : hs - 1, x1 = x0 + 1 < ws ? x0 + 1 : ws - 1;
        const float wy = fy - y0, wx = fx - x0;
        const float a00 = crop_texel<U>(base, y0 * pitch + (x0 << SH)), a01 = crop_texel<U>(base, y0 * pitch + (x1 << SH));
        const float a10 = crop_texel<U>(base, y1 * pitch + (x0 << SH)), a11 = crop_texel<U>(base, y1 * pitch + (x1 << SH));
        const float top = a00 + (a01 - a00) * wx, bot = a10 + (a11 - a10) * wx;
        yuv[0] = top + (bot - top) * wy;
    }
    const int hc = hs >> 1, wc = ws >> 1;
    float gx = p.siting == 0 ? fx * 0.5f : (fx - 0.5f) * 0.5f, gy = (fy - 0.5f) * 0.5f;
    gx = fminf(fmaxf(gx, 0.f), (float)(wc - 1));
    gy = fminf(fmaxf(gy, 0.f), (float)(hc - 1));
    const int y0 = min((int)gy, hc - 1), x0 = min((int)gx, wc - 1);
    const int y1 = min(y0 + 1, hc - 1), x1 = min(x0 + 1, wc - 1);
    const float wy = gy - y0, wx = gx - x0;
    const int c_pitch = __float_as_int(csc[12]), c_step = __float_as_int(csc[15]);
    const int o00 = y0 * c_pitch + x0 * c_step, o01 = y0 * c_pitch + x1 * c_step;
    const int o10 = y1 * c_pitch + x0 * c_step, o11 = y1 * c_pitch + x1 * c_step;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        int plane = __float_as_int(csc[13 + ch]);                 // one scalar base and a 32-bit offset per load
        // Cr's four offsets are formed once Cb is blended: with all eight chroma loads in flight beside luma's four the tap bodies
        // take 75 vector registers and the kernel drops from 7 waves a SIMD to 6 (71 this way; EXPERIMENTS.md)
        if (ch == 1) asm volatile("" : "+v"(plane) : "v"(yuv[1]));
        const float a00 = crop_texel<U>(base, plane + o00), a01 = crop_texel<U>(base, plane + o01);
        const float a10 = crop_texel<U>(base, plane + o10), a11 = crop_texel<U>(base, plane + o11);
        const float top = a00 + (a01 - a00) * wx, bot = a10 + (a11 - a10) * wx;
        yuv[1 + ch] = top + (bot - top) * wy;
    }
    const float e0 = yuv[0] - csc[9], e1 = yuv[1] - csc[10], e2 = yuv[2] - csc[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = fminf(fmaxf((csc[c * 3] * e0 + csc[c * 3 + 1] * e1) + csc[c * 3 + 2] * e2, 0.f), 255.f);
    return true;
}

__device__ __forceinline__ int crop_taps(float a, float b, int max_taps) {
    const float s = sqrtf(a * a + b * b);
    return s > 1.015625f && isfinite(s) ? min(max_taps, (int)ceilf(fminf(s, 64.f))) : 1;
}

// The pixels of one slot.  AREA = false is the plain crop, one sample at the pixel's centre: the loop the kernel always had, kept apart
// from the tap loops so that it compiles to what it was.  AREA = true: a live slot, kx x ky samples over the pixel's footprint.
// FMT (LH_FRAMES_*) picks the sample function, nothing else: the walk, the tap offsets, the accumulation and the store are shared.
template <int FMT>
__device__ __forceinline__ bool crop_sample_of(const CropArgs& p, const float* csc, const unsigned char* base, float fx, float fy, float s[3]) {
    if constexpr (FMT == LH_FRAMES_420) return crop_sample_420<unsigned char>(p, csc, base, fx, fy, s);
    else if constexpr (FMT == LH_FRAMES_420W) return crop_sample_420<unsigned short>(p, csc, base, fx, fy, s);
    else if constexpr (FMT == LH_FRAMES_NV12) return crop_sample_nv12(p, csc, base, fx, fy, s);
    else return crop_sample(base, p.hs, p.ws, fx, fy, s);
}

// JIT = LH_JIT_APPLY: ColorJitter between the sample and Normalize.  LH_JIT_MEAN: nothing is stored, the interior pixels' grey levels
// (after the ops in front of contrast) are summed in the order of the walk: the return value (0 otherwise).
template <typename T, bool AREA, int FMT, int JIT = LH_JIT_NONE>
__device__ __forceinline__ double crop_pixels(const CropArgs& p, const unsigned char* base, bool live, T* dst, int first, int stride,
                                            int per_slot, float m0, float m1, float m2, float m3, float m4, float m5, int kx, int ky,
                                            bool tiled, const float* csc = nullptr, const CropJit jit = {}) {
    const float fkx2 = (float)(2 * kx), fky2 = (float)(2 * ky), inv = 1.f / (float)(kx * ky);
    // AREA, tiled (the slot's choice, below): a wave takes an 8 x 8 tile of the output instead of 64 pixels of a row, so that its samples
    // stay within a square of the frame (a row of a turned ROI is a slanted line across many frame rows: a cache line per lane and load)
    const int tiles_x = (p.wp + 7) >> 3, n = AREA && tiled ? tiles_x * ((p.hp + 7) >> 3) * 64 : per_slot;
    double grey = 0.0;                                            // LH_JIT_MEAN only
    for (int q = first; q < n; q += stride) {
        int y, x;
        if (AREA && tiled) {
            const int tile = q >> 6, ty = tile / tiles_x;
            y = ty * 8 + ((q >> 3) & 7);
            x = (tile - ty * tiles_x) * 8 + (q & 7);
            if (y >= p.hp || x >= p.wp) continue;
        } else {
            y = q / p.wp;
            x = q - y * p.wp;
        }
        const int i = y * p.wp + x;
        const int oy = y - p.pad, ox = x - p.pad;
        float v[3] = {0.f, 0.f, 0.f};
        if ((unsigned)oy < (unsigned)p.h && (unsigned)ox < (unsigned)p.w) {
            float c[3] = {0.f, 0.f, 0.f};
            if constexpr (!AREA) {
                float s[3];
                if (live && crop_sample_of<FMT>(p, csc, base, (m0 * ox + m1 * oy) + m2, (m3 * ox + m4 * oy) + m5, s)) {   // NaN: black
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) c[ch] = s[ch] * (1.f / 255.f);
                }
            } else {
                float acc[3] = {0.f, 0.f, 0.f};
                for (int j = 0; j < ky; ++j) {
                    const float uy = (float)oy + (float)(2 * j + 1 - ky) / fky2;
                    for (int t = 0; t < kx; ++t) {
                        const float ux = (float)ox + (float)(2 * t + 1 - kx) / fkx2;
                        float s[3];
                        if (crop_sample_of<FMT>(p, csc, base, (m0 * ux + m1 * uy) + m2, (m3 * ux + m4 * uy) + m5, s)) {
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) acc[ch] += s[ch];
                        }
                    }
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch] = (acc[ch] * inv) * (1.f / 255.f);
            }
            if constexpr (JIT == LH_JIT_MEAN) {
                cj_apply(c, jit.f, jit.order, 0, jit.kc, 0.f);
                grey += (double)cj_gray(c);
            }
            if constexpr (JIT == LH_JIT_APPLY) cj_apply(c, jit.f, jit.order, 0, 4, jit.mean);          // black pixels are jittered too
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = (c[ch] - p.mean[ch]) * p.istd[ch];
        }
        if constexpr (JIT == LH_JIT_MEAN) continue;
        if constexpr (JIT == LH_JIT_APPLY || JIT == LH_JIT_STORE) {      // the fp32 instantiation stores for all three dtypes (uniform)
            if (jit.dtype == LH_BF16) crop_store((bf16*)dst, i, v);
            else if (jit.dtype == LH_F16) crop_store((f16*)dst, i, v);
            else crop_store((float*)dst, i, v);
        } else {
            crop_store(dst, i, v);
        }
    }
    return grey;
}

// ------------------------------------------------------------------------------------------------ ROI augmentation (training on frames)
// The caller's ROI and this step's draw aug = (c, s, k, tx, ty, flip) -> the ROI that lh_roi_affine turns into the crop matrix: the
// centre moves by (tx, ty) extents along the ROI's own axes, the extents grow by k, the direction turns by (c, s) = (cos, sin) of the
// drawn angle and flip toggles the mirror.  One thread per slot, fp32 in this order; topdown.py's roi_perturb_host restates it.
// (A mode of frames_crop_kernel<float>, launched by lh_roi_perturb: CropArgs.)
//     bw = x1-x0, bh = y1-y0, cx = (x0+x1)*0.5, cy = (y0+y1)*0.5,  n = sqrtf(rx*rx + ry*ry), ux = rx/n, uy = ry/n
//     dx = tx*bw, dy = ty*bh,  cx' = cx + (dx*ux - dy*uy), cy' = cy + (dx*uy + dy*ux)
//     hw = (bw*k)*0.5, hh = (bh*k)*0.5,  box' = (cx'-hw, cy'-hh, cx'+hw, cy'+hh)
//     rot' = (ux*c - uy*s, ux*s + uy*c),  mirror' = (mirror != 0) != (flip != 0)
// A row that is exactly (1, 0, 1, 0, 0, 0) copies box, rot and mirror bit for bit (rot is NOT normalised): no augmentation is the
// un-augmented crop.  A box, rot or aug row that is not finite, or n not > 0, copies them as well: lh_roi_affine empties such a slot.
__device__ __forceinline__ void roi_perturb_slot(int i, const float* boxes, const float* rot, const int* mirror, const float* aug,
                                                 float* boxes_out, float* rot_out, int* mirror_out) {
    const float x0 = boxes[i * 4], y0 = boxes[i * 4 + 1], x1 = boxes[i * 4 + 2], y1 = boxes[i * 4 + 3];
    const float rx = rot ? rot[i * 2] : 1.f, ry = rot ? rot[i * 2 + 1] : 0.f;
    const int mi = mirror ? mirror[i] : 0;
    const float* a = aug + i * 6;
    const float c = a[0], s = a[1], k = a[2], tx = a[3], ty = a[4], flip = a[5];
    const float n = sqrtf(rx * rx + ry * ry);
    const bool same = c == 1.f && s == 0.f && k == 1.f && tx == 0.f && ty == 0.f && flip == 0.f;
    const bool ok = isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && isfinite(rx) && isfinite(ry) && n > 0.f && isfinite(c)
                    && isfinite(s) && isfinite(k) && isfinite(tx) && isfinite(ty) && isfinite(flip);
    if (same || !ok) {
        boxes_out[i * 4] = x0; boxes_out[i * 4 + 1] = y0; boxes_out[i * 4 + 2] = x1; boxes_out[i * 4 + 3] = y1;
        rot_out[i * 2] = rx; rot_out[i * 2 + 1] = ry;
        mirror_out[i] = mi;
        return;
    }
    const float bw = x1 - x0, bh = y1 - y0;
    const float cx = (x0 + x1) * 0.5f, cy = (y0 + y1) * 0.5f;
    const float ux = rx / n, uy = ry / n;
    const float dx = tx * bw, dy = ty * bh;
    const float ncx = cx + (dx * ux - dy * uy), ncy = cy + (dx * uy + dy * ux);
    const float hw = (bw * k) * 0.5f, hh = (bh * k) * 0.5f;
    boxes_out[i * 4] = ncx - hw; boxes_out[i * 4 + 1] = ncy - hh; boxes_out[i * 4 + 2] = ncx + hw; boxes_out[i * 4 + 3] = ncy + hh;
    rot_out[i * 2] = ux * c - uy * s; rot_out[i * 2 + 1] = ux * s + uy * c;
    mirror_out[i] = ((mi != 0) != (flip != 0.f)) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ frame -> crop for the joints
// The twin of lh_affine_points: frame coordinates through the INVERSE of the slot's crop matrix (crop -> frame), so that the target of
// a training step on frames is rendered where the crop kernel put the hand.  One thread per point, fp32 in this order
// (topdown.py: affine_points_inv_host):
//     det = m0*m4 - m1*m3, qx = x - m2, qy = y - m5,  ox = (m4*qx - m1*qy) / det, oy = (m0*qy - m3*qx) / det
// An empty slot (src_frame < 0), or det not finite or == 0, writes (LH_POINT_OFF, LH_POINT_OFF): off every target renderer's map.
// The matrix (1, 0, 0, 0, 1, 0) returns the points' own bits.  Columns past the first two are neither read nor written.
// (The other mode of frames_crop_kernel<float>, launched by lh_affine_points_inv.)
__device__ __forceinline__ void affine_points_inv_point(int i, const float* pts, int pstride, const float* mat, const int* src_frame,
                                                        float* out, int ostride, int j) {
    const int slot = i / j;
    const float* m = mat + slot * 6;
    const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const float det = m0 * m4 - m1 * m3;
    float ox = LH_POINT_OFF, oy = LH_POINT_OFF;
    if (src_frame[slot] >= 0 && isfinite(det) && det != 0.f) {
        const float qx = pts[(long)i * pstride] - m2, qy = pts[(long)i * pstride + 1] - m5;
        ox = (m4 * qx - m1 * qy) / det;
        oy = (m0 * qy - m3 * qx) / det;
    }
    out[(long)i * ostride] = ox;
    out[(long)i * ostride + 1] = oy;
}

// The modes' thread: one slot or one point.
__device__ __forceinline__ void crop_aux_modes(const CropArgs& p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    if (p.op == LH_CROP_ROI_PERTURB) roi_perturb_slot(i, p.in0, p.in1, p.iin, p.in2, p.out0, p.out1, p.iout);
    else affine_points_inv_point(i, p.in0, p.pstride, p.in1, p.iin, p.out0, p.ostride, p.j);
}

// One slot's pixels through the body its format (LH_FRAMES_*) and tap counts select; JIT as in crop_pixels.
template <typename T, int JIT>
__device__ __forceinline__ double crop_slot(const CropArgs& p, const unsigned char* base, bool live, int fmt, T* dst, int first, int stride,
                                          int per_slot, float m0, float m1, float m2, float m3, float m4, float m5, int kx, int ky, bool tiled,
                                          const CropJit jit) {
    if (fmt != LH_FRAMES_RGB) {
        // the 12 coefficients live in vector registers: as scalars they take the kernel past 100 SGPRs, and the RGB entries, which never
        // read them, from 8 waves a SIMD to 7 (measured on the turned legs of tools/topdown_cost.py: EXPERIMENTS.md)
        float csc[sizeof(T) == 4 ? 16 : 12];
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            csc[c] = c < 9 ? p.k[c] : p.o[c - 9];
            asm volatile("" : "+v"(csc[c]));
        }
        if constexpr (sizeof(T) == 4) {                           // the plane descriptor: the fp32 instantiation's alone
            if (fmt >= LH_FRAMES_420) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    csc[12 + c] = __int_as_float(p.dsc[c]);
                    asm volatile("" : "+v"(csc[12 + c]));
                }
                if (fmt == LH_FRAMES_420) {
                    if (kx * ky == 1) return crop_pixels<T, false, LH_FRAMES_420, JIT>(p, base, live, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, 1, 1, false, csc, jit);
                    return crop_pixels<T, true, LH_FRAMES_420, JIT>(p, base, live, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, kx, ky, tiled, csc, jit);
                }
                if (kx * ky == 1) return crop_pixels<T, false, LH_FRAMES_420W, JIT>(p, base, live, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, 1, 1, false, csc, jit);
                return crop_pixels<T, true, LH_FRAMES_420W, JIT>(p, base, live, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, kx, ky, tiled, csc, jit);
            }
        }
        if (kx * ky == 1) return crop_pixels<T, false, LH_FRAMES_NV12, JIT>(p, base, live, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, 1, 1, false, csc, jit);
        return crop_pixels<T, true, LH_FRAMES_NV12, JIT>(p, base, live, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, kx, ky, tiled, csc, jit);
    }
    if (kx * ky == 1) return crop_pixels<T, false, LH_FRAMES_RGB, JIT>(p, base, live, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, 1, 1, false, nullptr, jit);
    return crop_pixels<T, true, LH_FRAMES_RGB, JIT>(p, base, live, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, kx, ky, tiled, nullptr, jit);
}

template <typename T>
__global__ __launch_bounds__(256) void frames_crop_kernel(const CropArgs p) {
    if constexpr (sizeof(T) == 4) {                               // the fp32 instantiation alone carries the modes (CropArgs)
        if (p.op == LH_CROP_ROI_PERTURB || p.op == LH_CROP_POINTS_INV) {
            crop_aux_modes(p);
            return;
        }
    }
    const int slot = blockIdx.y;
    const float* m = p.mat + slot * 6;
    const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const int sf = p.src_frame[slot];
    bool live = sf >= 0 && sf < p.n_frames;                       // anything else is an empty slot: never an address
    const bool nv12 = p.format == LH_FRAMES_NV12;                 // workgroup-uniform: one branch in front of the pixel loops
    int fmt = nv12 ? LH_FRAMES_NV12 : LH_FRAMES_RGB;
    const unsigned char* base = p.src + (nv12 ? (long)(live ? sf : 0) * p.frame_stride : (long)(live ? sf : 0) * p.hs * p.ws * 3);
    if constexpr (sizeof(T) == 4) {
        if (p.gen) {                                              // the surfaces entry: where the frame is, and which sample reads it
            fmt = p.format;
            if (p.table) {
                const long long at = live ? p.table[sf] : 0;      // a scalar load; tested before it becomes an address
                live = live && at != 0;
                base = reinterpret_cast<const unsigned char*>(live ? at : 0);
            } else {
                base = p.src + (long)(live ? sf : 0) * p.frame_stride;
            }
        }
    }
    const int per_slot = p.hp * p.wp;
    T* dst = (T*)p.dst + (long)slot * per_slot * 4;
    int kx = 1, ky = 1;                                           // workgroup-uniform; the plain entry never pays for the square roots
    if (p.max_taps > 1 && live) { kx = crop_taps(m0, m3, p.max_taps); ky = crop_taps(m1, m4, p.max_taps); }
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    // 64 pixels of a crop row cross 64 * |m3| frame rows: from 16 on the tiled walk reads fewer cache lines per load (measured: EXPERIMENTS.md)
    const bool tiled = fabsf(m3) >= 0.25f;
    if constexpr (sizeof(T) == 4) {
        // ColorJitter: both launches are this instantiation's, whatever the crop's dtype -- the samples are fp32 in all three, only the
        // store differs -- so the 16-bit instantiations keep the code, registers and occupancy they had
        if (p.op == LH_CROP_GREY_MEAN) {                          // grid (CJ_STRIPS, b): workgroup blockIdx.x of the slot writes partial blockIdx.x
            __shared__ double red[256];
            CropJit jit = {p.jfactors + slot * 4, p.jorder + slot * 4, 0.f, 4, LH_F32};
            for (int k = 3; k >= 0; --k)                          // position of the contrast op (4 = absent)
                if (jit.order[k] == 1) jit.kc = k;
            if (jit.kc == 4) {                                    // workgroup-uniform: nothing to reduce, nothing is sampled
                if (threadIdx.x == 0) p.jpartial[slot * CJ_STRIPS + blockIdx.x] = 0.0;
                return;
            }
            red[threadIdx.x] = crop_slot<T, LH_JIT_MEAN>(p, base, live, fmt, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, kx, ky, tiled, jit);
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
                __syncthreads();
            }
            if (threadIdx.x == 0) p.jpartial[slot * CJ_STRIPS + blockIdx.x] = red[0];
            return;
        }
        if (p.jfactors) {                                         // workgroup-uniform, as format: the entries without ColorJitter run the bodies below
            double sum = 0.0;                                     // once per workgroup (uniform addresses), never per pixel
            for (int k = 0; k < CJ_STRIPS; ++k) sum += p.jpartial[slot * CJ_STRIPS + k];
            const CropJit jit = {p.jfactors + slot * 4, p.jorder + slot * 4, (float)(sum / ((double)p.h * p.w)), 4, p.jdtype};
            T* out = (T*)((char*)p.dst + (long)slot * per_slot * (p.jdtype == LH_F32 ? 16 : 8));      // the slot's pixels in dst's dtype
            crop_slot<T, LH_JIT_APPLY>(p, base, live, fmt, out, first, stride, per_slot, m0, m1, m2, m3, m4, m5, kx, ky, tiled, jit);
            return;
        }
        if (p.gen) {                                              // the surfaces entry without ColorJitter: this instantiation stores in jdtype
            const CropJit jit = {nullptr, nullptr, 0.f, 4, p.jdtype};
            T* out = (T*)((char*)p.dst + (long)slot * per_slot * (p.jdtype == LH_F32 ? 16 : 8));
            crop_slot<T, LH_JIT_STORE>(p, base, live, fmt, out, first, stride, per_slot, m0, m1, m2, m3, m4, m5, kx, ky, tiled, jit);
            return;
        }
    }
    crop_slot<T, LH_JIT_NONE>(p, base, live, fmt, dst, first, stride, per_slot, m0, m1, m2, m3, m4, m5, kx, ky, tiled, CropJit{});
}

// What the NV12 entry adds to the RGB ones' arguments.
struct Nv12Layout {
    int pitch, uv_offset;
    long frame_stride;
    int siting;
    const float* csc12;
};

// What the ColorJitter entry adds: the per-slot draw and the grey-mean partials (lh_frames_crop_jitter_workspace_bytes).
struct CropJitter {
    const float* factors;
    const int* order;
    void* workspace;
};

// All entries: ``who`` names the entry in the error text, max_taps = 1 is the plain crop, yuv = nullptr packed RGB frames, jitter =
// nullptr no ColorJitter (one launch; with it the grey-mean launch goes first).
static int frames_crop_launch(const char* who, const unsigned char* frames_u8, void* out, int b, int n_frames, int hs, int ws, int h, int w,
                              int pad, int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                              int max_taps, int dtype, void* stream, const Nv12Layout* yuv = nullptr, const CropJitter* jitter = nullptr) {
    LH_REQUIRE(!jitter || (jitter->factors && jitter->order && jitter->workspace), "%s: bad arguments (factors_dev, order_dev or workspace is null)",
               who);
    LH_REQUIRE(!jitter || ((uintptr_t)jitter->workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    LH_REQUIRE(frames_u8 && out && mean3 && std3 && mat_dev && src_frame_dev && b > 0 && b <= 65535 && n_frames > 0 && hs > 0 && ws > 0
               && h > 0 && w > 0 && pad >= 0 && wp >= w + 2 * pad, "%s: bad arguments", who);
    LH_REQUIRE(max_taps >= 1 && max_taps <= 8, "%s: max_taps must be 1..8, not %d", who, max_taps);
    LH_REQUIRE(lh_dtype_size(dtype) > 0, "%s: unsupported dtype %d", who, dtype);
    LH_REQUIRE(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", who);
    CropArgs a;
    a.src = frames_u8; a.dst = out; a.mat = mat_dev; a.src_frame = src_frame_dev;
    a.n_frames = n_frames; a.hs = hs; a.ws = ws; a.h = h; a.w = w; a.pad = pad; a.hp = h + 2 * pad; a.wp = wp;
    a.max_taps = max_taps;
    a.op = LH_CROP; a.n = a.j = a.pstride = a.ostride = 0;
    a.in0 = a.in1 = a.in2 = nullptr; a.iin = nullptr; a.out0 = a.out1 = nullptr; a.iout = nullptr;
    a.jfactors = nullptr; a.jorder = nullptr; a.jpartial = nullptr; a.jdtype = dtype;
    a.gen = 0; a.table = nullptr; a.dsc[0] = a.dsc[1] = a.dsc[2] = a.dsc[3] = 0;
    a.format = yuv ? LH_FRAMES_NV12 : LH_FRAMES_RGB;
    a.pitch = a.uv_offset = a.siting = 0; a.frame_stride = 0;
    for (int c = 0; c < 9; ++c) a.k[c] = 0.f;
    a.o[0] = a.o[1] = a.o[2] = 0.f;
    // one slot's pixels and one frame's bytes are 32-bit quantities; the frame BUFFER is indexed with long (64 frames of 1080p pass 2^31)
    LH_REQUIRE((long)a.hp * wp < (1L << 29) && (yuv || (long)hs * ws * 3 < (1L << 31)), "%s: crop or frame too large for 32-bit pixel indices",
               who);
    if (yuv) {
        LH_REQUIRE(yuv->csc12, "%s: bad arguments", who);
        LH_REQUIRE(hs >= 2 && ws >= 2 && hs % 2 == 0 && ws % 2 == 0, "%s: NV12 frames have even sides >= 2, not %d x %d", who, hs, ws);
        LH_REQUIRE(yuv->pitch >= ws, "%s: pitch %d is below the frame's width %d", who, yuv->pitch, ws);
        LH_REQUIRE(yuv->uv_offset >= (long)yuv->pitch * hs, "%s: uv_offset %d lies inside the luma plane (pitch * hs = %ld)", who,
                   yuv->uv_offset, (long)yuv->pitch * hs);
        LH_REQUIRE(yuv->frame_stride < (1L << 31), "%s: frame_stride %ld does not fit 32-bit byte indices", who, yuv->frame_stride);
        LH_REQUIRE(yuv->uv_offset + (long)(hs / 2 - 1) * yuv->pitch + ws <= yuv->frame_stride,
                   "%s: the chroma plane (uv_offset %d, %d rows of pitch %d) does not end inside frame_stride %ld", who, yuv->uv_offset, hs / 2,
                   yuv->pitch, yuv->frame_stride);
        LH_REQUIRE(yuv->siting == 0 || yuv->siting == 1, "%s: chroma_siting must be 0 (left) or 1 (center), not %d", who, yuv->siting);
        for (int c = 0; c < 12; ++c) LH_REQUIRE(yuv->csc12[c] - yuv->csc12[c] == 0.f, "%s: csc12[%d] is not finite", who, c);
        a.pitch = yuv->pitch; a.uv_offset = yuv->uv_offset; a.frame_stride = yuv->frame_stride; a.siting = yuv->siting;
        for (int c = 0; c < 9; ++c) a.k[c] = yuv->csc12[c];
        for (int c = 0; c < 3; ++c) a.o[c] = yuv->csc12[9 + c];
    }
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.istd[c] = 1.f / std3[c]; }
    const int chunks = lh_grid((long)a.hp * wp, 1024);
    if (jitter) {
        a.jfactors = jitter->factors; a.jorder = jitter->order; a.jpartial = (double*)jitter->workspace;
        a.op = LH_CROP_GREY_MEAN;                                 // the samples are fp32 whatever the crop's dtype is
        hipLaunchKernelGGL((frames_crop_kernel<float>), dim3(CJ_STRIPS, b), dim3(256), 0, (hipStream_t)stream, a);
        LH_LAUNCH_CHECK("frames_crop_jitter_to_nhwc4 grey-mean launch");
        a.op = LH_CROP;                                           // the apply mode: jfactors is set, the store is a.jdtype's
        hipLaunchKernelGGL((frames_crop_kernel<float>), dim3(chunks, b), dim3(256), 0, (hipStream_t)stream, a);
        LH_LAUNCH_CHECK("frames_crop_jitter_to_nhwc4 launch");
        return LH_OK;
    }
    LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((frames_crop_kernel<T>), dim3(chunks, b), dim3(256), 0, (hipStream_t)stream, a));
    LH_LAUNCH_CHECK(yuv ? "frames_crop_yuv_to_nhwc4 launch" : max_taps > 1 ? "frames_crop_area_to_nhwc4 launch" : "frames_crop_to_nhwc4 launch");
    return LH_OK;
}

extern "C" int lh_frames_crop_to_nhwc4(const unsigned char* frames_u8, void* out, int b, int n_frames, int hs, int ws, int h, int w, int pad,
                                       int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                                       int dtype, void* stream) {
    return frames_crop_launch("lh_frames_crop_to_nhwc4", frames_u8, out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev,
                              src_frame_dev, 1, dtype, stream);
}

extern "C" int lh_frames_crop_area_to_nhwc4(const unsigned char* frames_u8, void* out, int b, int n_frames, int hs, int ws, int h, int w,
                                            int pad, int wp, const float* mean3, const float* std3, const float* mat_dev,
                                            const int* src_frame_dev, int max_taps, int dtype, void* stream) {
    return frames_crop_launch("lh_frames_crop_area_to_nhwc4", frames_u8, out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev,
                              src_frame_dev, max_taps, dtype, stream);
}

extern "C" int lh_frames_crop_yuv_to_nhwc4(const unsigned char* frames_nv12, void* out, int b, int n_frames, int hs, int ws, int pitch,
                                           int uv_offset, long frame_stride, int chroma_siting, const float* csc12, int h, int w, int pad,
                                           int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                                           int max_taps, int dtype, void* stream) {
    const Nv12Layout yuv = {pitch, uv_offset, frame_stride, chroma_siting, csc12};
    return frames_crop_launch("lh_frames_crop_yuv_to_nhwc4", frames_nv12, out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev,
                              src_frame_dev, max_taps, dtype, stream, &yuv);
}

extern "C" size_t lh_frames_crop_jitter_workspace_bytes(int b) { return b > 0 ? (size_t)b * CJ_STRIPS * sizeof(double) : 0; }

extern "C" int lh_frames_crop_jitter_to_nhwc4(const unsigned char* frames, void* out, int b, int n_frames, int hs, int ws, int pitch,
                                              int uv_offset, long frame_stride, int chroma_siting, const float* csc12, int h, int w, int pad,
                                              int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                                              int max_taps, const float* factors_dev, const int* order_dev, void* workspace, int dtype,
                                              void* stream) {
    const Nv12Layout yuv = {pitch, uv_offset, frame_stride, chroma_siting, csc12};
    const CropJitter jitter = {factors_dev, order_dev, workspace};
    return frames_crop_launch("lh_frames_crop_jitter_to_nhwc4", frames, out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev,
                              src_frame_dev, max_taps, dtype, stream, csc12 ? &yuv : nullptr, &jitter);
}

// ------------------------------------------------------------------------------------------------ decoder surfaces, 4:2:0 flavours
// The entry of the surface table and the plane descriptor (the header comment).  Every launch is the fp32 instantiation's, which
// stores in ``dtype``.  All of the layout is checked here, in front of any launch: the kernel trusts it.
extern "C" int lh_frames_crop_surfaces_to_nhwc4(const unsigned char* frames, void* out, long frame_stride, const long long* surface_table_dev,
                                                const lh_frames_layout* layout, int b, int n_frames, int hs, int ws, int h, int w,
                                                int pad, int wp, const float* mean3, const float* std3, const float* mat_dev,
                                                const int* src_frame_dev, int max_taps, const float* factors_dev, const int* order_dev,
                                                void* workspace, int dtype, void* stream) {
    const char* who = "lh_frames_crop_surfaces_to_nhwc4";
    LH_REQUIRE(frames || surface_table_dev, "%s: no frame source (frames and surface_table_dev are both null)", who);
    LH_REQUIRE(!(frames && surface_table_dev), "%s: two frame sources (pass frames or surface_table_dev, not both)", who);
    LH_REQUIRE(layout && out && mean3 && std3 && mat_dev && src_frame_dev && b > 0 && b <= 65535 && n_frames > 0 && hs > 0 && ws > 0 && h > 0
               && w > 0 && pad >= 0 && wp >= w + 2 * pad, "%s: bad arguments", who);
    const bool jitter = factors_dev || order_dev || workspace;
    LH_REQUIRE(!jitter || (factors_dev && order_dev && workspace), "%s: bad arguments (factors_dev, order_dev or workspace is null)", who);
    LH_REQUIRE(!jitter || ((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    LH_REQUIRE(max_taps >= 1 && max_taps <= 8, "%s: max_taps must be 1..8, not %d", who, max_taps);
    LH_REQUIRE(lh_dtype_size(dtype) > 0, "%s: unsupported dtype %d", who, dtype);
    LH_REQUIRE(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", who);
    LH_REQUIRE(!surface_table_dev || ((uintptr_t)surface_table_dev & 7) == 0, "%s: surface_table_dev must be 8-byte aligned", who);
    LH_REQUIRE((long)(h + 2 * pad) * wp < (1L << 29), "%s: crop too large for 32-bit pixel indices", who);
    const int f = layout->format;
    LH_REQUIRE(f >= LH_FRAMES_FMT_RGB && f <= LH_FRAMES_FMT_P010, "%s: unknown format code %d", who, f);
    CropArgs a = {};
    a.src = frames; a.table = surface_table_dev; a.gen = 1;
    a.dst = out; a.mat = mat_dev; a.src_frame = src_frame_dev;
    a.n_frames = n_frames; a.hs = hs; a.ws = ws; a.h = h; a.w = w; a.pad = pad; a.hp = h + 2 * pad; a.wp = wp;
    a.max_taps = max_taps; a.op = LH_CROP; a.jdtype = dtype;
    long need;                                                    // the highest byte a sample can touch, plus one
    if (f == LH_FRAMES_FMT_RGB) {
        need = (long)hs * ws * 3;
        a.format = LH_FRAMES_RGB;
    } else {
        const int sb = f == LH_FRAMES_FMT_P010 ? 2 : 1, hc = hs / 2, wc = ws / 2;
        const long pitch = layout->pitch, c_pitch = layout->c_pitch, cb = layout->cb_offset, cr = layout->cr_offset;
        LH_REQUIRE(hs >= 2 && ws >= 2 && hs % 2 == 0 && ws % 2 == 0, "%s: 4:2:0 frames have even sides >= 2, not %d x %d", who, hs, ws);
        LH_REQUIRE(pitch >= (long)ws * sb, "%s: pitch %ld is below a luma row's %ld bytes", who, pitch, (long)ws * sb);
        const bool planar = f == LH_FRAMES_FMT_YUV420P;
        const long c_row = planar ? wc : (long)wc * 2 * sb;       // the bytes of one chroma row that are samples
        LH_REQUIRE(c_pitch >= c_row, "%s: c_pitch %ld is below a chroma row's %ld bytes", who, c_pitch, c_row);
        LH_REQUIRE(f != LH_FRAMES_FMT_NV12 || cr == cb + 1, "%s: nv12 has cr_offset = cb_offset + 1, not %ld / %ld", who, cb, cr);
        LH_REQUIRE(f != LH_FRAMES_FMT_NV21 || cb == cr + 1, "%s: nv21 has cb_offset = cr_offset + 1, not %ld / %ld", who, cb, cr);
        LH_REQUIRE(f != LH_FRAMES_FMT_P010 || cr == cb + 2, "%s: p010 has cr_offset = cb_offset + 2, not %ld / %ld", who, cb, cr);
        LH_REQUIRE(sb == 1 || (pitch % 2 == 0 && c_pitch % 2 == 0 && cb % 2 == 0 && cr % 2 == 0),
                   "%s: p010 samples are 16-bit: pitch %ld, c_pitch %ld, cb_offset %ld and cr_offset %ld must be even", who, pitch, c_pitch, cb, cr);
        const long luma_end = (long)(hs - 1) * pitch + (long)ws * sb;
        const long c_lo = cb < cr ? cb : cr, c_hi = cb < cr ? cr : cb;
        LH_REQUIRE(c_lo >= luma_end, "%s: a chroma plane (cb_offset %ld, cr_offset %ld) lies inside the luma plane (%ld bytes)", who, cb, cr,
                   luma_end);
        const long plane = (long)(hc - 1) * c_pitch + (planar ? wc : (long)(wc - 1) * 2 * sb + sb);      // one plane's extent from its offset
        LH_REQUIRE(!planar || c_hi >= c_lo + plane, "%s: the chroma planes overlap (cb_offset %ld, cr_offset %ld, %ld bytes each)", who, cb, cr,
                   plane);
        need = c_hi + plane;
        LH_REQUIRE(layout->frame_bytes >= need && need < (1L << 31), "%s: the planes end at byte %ld, outside frame_bytes %d (< 2^31)", who, need,
                   layout->frame_bytes);
        LH_REQUIRE(layout->chroma_siting == 0 || layout->chroma_siting == 1, "%s: chroma_siting must be 0 (left) or 1 (center), not %d", who,
                   layout->chroma_siting);
        for (int c = 0; c < 12; ++c) LH_REQUIRE(layout->csc12[c] - layout->csc12[c] == 0.f, "%s: csc12[%d] is not finite", who, c);
        a.format = sb == 2 ? LH_FRAMES_420W : LH_FRAMES_420;
        a.pitch = (int)pitch; a.siting = layout->chroma_siting;
        a.dsc[0] = (int)c_pitch; a.dsc[1] = (int)cb; a.dsc[2] = (int)cr; a.dsc[3] = planar ? 1 : 2 * sb;
        for (int c = 0; c < 9; ++c) a.k[c] = layout->csc12[c];
        for (int c = 0; c < 3; ++c) a.o[c] = layout->csc12[9 + c];
        LH_REQUIRE(sb == 1 || !frames || (((uintptr_t)frames | (uintptr_t)frame_stride) & 1) == 0,
                   "%s: p010 samples are 16-bit: frames and frame_stride must be even", who);
    }
    LH_REQUIRE(need < (1L << 31), "%s: a frame of %ld bytes does not fit 32-bit byte indices", who, need);
    LH_REQUIRE(!frames || frame_stride >= need, "%s: frame_stride %ld is below the %ld bytes a frame's samples span", who, frame_stride, need);
    a.frame_stride = frames ? frame_stride : 0;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.istd[c] = 1.f / std3[c]; }
    const int chunks = lh_grid((long)a.hp * wp, 1024);
    if (jitter) {
        a.jfactors = factors_dev; a.jorder = order_dev; a.jpartial = (double*)workspace;
        a.op = LH_CROP_GREY_MEAN;
        hipLaunchKernelGGL((frames_crop_kernel<float>), dim3(CJ_STRIPS, b), dim3(256), 0, (hipStream_t)stream, a);
        LH_LAUNCH_CHECK("frames_crop_surfaces_to_nhwc4 grey-mean launch");
        a.op = LH_CROP;
    }
    hipLaunchKernelGGL((frames_crop_kernel<float>), dim3(chunks, b), dim3(256), 0, (hipStream_t)stream, a);
    LH_LAUNCH_CHECK("frames_crop_surfaces_to_nhwc4 launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ training on frames: the two modes
extern "C" int lh_roi_perturb(const float* boxes_dev, const float* rot_dev, const int* mirror_dev, const float* aug_dev, int b,
                              float* boxes_out, float* rot_out, int* mirror_out, void* stream) {
    LH_REQUIRE(boxes_dev && aug_dev && boxes_out && rot_out && mirror_out && b > 0, "lh_roi_perturb: bad arguments");
    LH_REQUIRE(boxes_out != boxes_dev && rot_out != rot_dev && mirror_out != mirror_dev && (const void*)boxes_out != (const void*)aug_dev
               && (const void*)rot_out != (const void*)aug_dev && (const void*)rot_out != (const void*)boxes_dev
               && (const void*)boxes_out != (const void*)rot_dev, "lh_roi_perturb: the outputs must not alias the inputs");
    CropArgs a = {};
    a.op = LH_CROP_ROI_PERTURB; a.n = b;
    a.in0 = boxes_dev; a.in1 = rot_dev; a.in2 = aug_dev; a.iin = mirror_dev; a.out0 = boxes_out; a.out1 = rot_out; a.iout = mirror_out;
    hipLaunchKernelGGL((frames_crop_kernel<float>), dim3((b + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    LH_LAUNCH_CHECK("roi_perturb launch");
    return LH_OK;
}


extern "C" int lh_affine_points_inv(const float* pts, int pstride, const float* mat_dev, const int* src_frame_dev, float* out, int ostride,
                                    int b, int j, void* stream) {
    LH_REQUIRE(pts && mat_dev && src_frame_dev && out && pstride >= 2 && ostride >= 2 && b > 0 && j > 0 && (long)b * j < (1L << 30),
               "lh_affine_points_inv: bad arguments");
    CropArgs a = {};
    a.op = LH_CROP_POINTS_INV; a.n = b * j; a.j = j; a.pstride = pstride; a.ostride = ostride;
    a.in0 = pts; a.in1 = mat_dev; a.iin = src_frame_dev; a.out0 = out;
    hipLaunchKernelGGL((frames_crop_kernel<float>), dim3((b * j + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    LH_LAUNCH_CHECK("affine_points_inv launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ keypoints -> next box
// One thread per slot walks its joints in order: comparisons and a widening about the centre, no atomics, so a replay is bit-reproducible.
__global__ void keypoints_to_boxes_kernel(const float* preds, const float* maxvals, const float* boxes, const int* src_frame, int b, int j,
                                          float min_score, int min_joints, float min_side, float* next_boxes, int* lost) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b) return;
    float lo_x = 0.f, lo_y = 0.f, hi_x = 0.f, hi_y = 0.f;
    int n = 0;
    for (int k = 0; k < j; ++k) {
        if (!(maxvals[(long)i * j + k] >= min_score)) continue;
        const float x = preds[((long)i * j + k) * 2], y = preds[((long)i * j + k) * 2 + 1];
        if (n == 0) { lo_x = hi_x = x; lo_y = hi_y = y; }
        lo_x = x < lo_x ? x : lo_x; hi_x = x > hi_x ? x : hi_x;
        lo_y = y < lo_y ? y : lo_y; hi_y = y > hi_y ? y : hi_y;
        ++n;
    }
    float* o = next_boxes + i * 4;
    if (n < min_joints || src_frame[i] < 0) {                     // too few confident joints, or nothing was cropped: keep the box
        o[0] = boxes[i * 4]; o[1] = boxes[i * 4 + 1]; o[2] = boxes[i * 4 + 2]; o[3] = boxes[i * 4 + 3];
        lost[i] = 1;
        return;
    }
    if (hi_x - lo_x < min_side) { const float c = (lo_x + hi_x) * 0.5f; lo_x = c - min_side * 0.5f; hi_x = c + min_side * 0.5f; }
    if (hi_y - lo_y < min_side) { const float c = (lo_y + hi_y) * 0.5f; lo_y = c - min_side * 0.5f; hi_y = c + min_side * 0.5f; }
    o[0] = lo_x; o[1] = lo_y; o[2] = hi_x; o[3] = hi_y;
    lost[i] = 0;
}

extern "C" int lh_keypoints_to_boxes(const float* preds_dev, const float* maxvals_dev, const float* boxes_dev, const int* src_frame_dev, int b,
                                     int j, float min_score, int min_joints, float min_side, float* next_boxes_dev, int* lost_dev, void* stream) {
    LH_REQUIRE(preds_dev && maxvals_dev && boxes_dev && src_frame_dev && next_boxes_dev && lost_dev && b > 0 && j > 0 && min_joints >= 1
               && (long)b * j < (1L << 30) && min_side >= 0.f && min_side <= 3.0e38f && min_score == min_score && next_boxes_dev != boxes_dev,
               "lh_keypoints_to_boxes: bad arguments");
    hipLaunchKernelGGL(keypoints_to_boxes_kernel, dim3((b + 63) / 64), dim3(64), 0, (hipStream_t)stream, preds_dev, maxvals_dev, boxes_dev,
                       src_frame_dev, b, j, min_score, min_joints, min_side, next_boxes_dev, lost_dev);
    LH_LAUNCH_CHECK("keypoints_to_boxes launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ oriented, mirrored ROI -> matrix
// The oriented sibling of box_affine_kernel: the box gives the ROI's centre and its extents along the ROI's own axes, rot = (rx, ry) is
// the frame direction of the crop's +x axis (any length, (1, 0) = upright) and mirror flips the crop's x axis, so a left hand reaches
// the network as a right one.  The matrix still takes a crop pixel index to a frame pixel index, so the crop kernel and
// lh_affine_points serve unchanged.  The crop's centre ((w-1)/2, (h-1)/2) lands on the box's centre.  No sinf / cosf: a direction.
__global__ void roi_affine_kernel(const float* boxes, const float* rot, const int* mirror, const int* frame_index, int b, int n_frames,
                                  float h, float w, float padding, float* mat, int* src_frame) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b) return;
    const float x0 = boxes[i * 4], y0 = boxes[i * 4 + 1], x1 = boxes[i * 4 + 2], y1 = boxes[i * 4 + 3];
    const float rx = rot[i * 2], ry = rot[i * 2 + 1];
    const int fi = frame_index[i];
    const float bw = x1 - x0, bh = y1 - y0;
    const float n = sqrtf(rx * rx + ry * ry);
    const bool ok = fi >= 0 && fi < n_frames && isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && bw > 0.f && bh > 0.f
                    && isfinite(rx) && isfinite(ry) && n > 0.f;
    float* m = mat + i * 6;
    if (!ok) {                                                    // an empty slot, as box_affine_kernel's
        src_frame[i] = -1;
        m[0] = m[1] = m[2] = m[3] = m[4] = m[5] = 0.f;
        return;
    }
    const float cx = (x0 + x1) * 0.5f, cy = (y0 + y1) * 0.5f;
    const float sw = padding * fmaxf(bw, bh * w / h), a = sw / w;
    const float c = rx / n, s = ry / n;
    const float ac = a * c, as = a * s, g = mirror[i] ? -1.f : 1.f;
    const float m0 = g * ac, m1 = -as, m3 = g * as, m4 = ac;
    const float hx = (w - 1.f) * 0.5f, hy = (h - 1.f) * 0.5f;
    src_frame[i] = fi;
    m[0] = m0; m[1] = m1; m[2] = cx - (m0 * hx + m1 * hy);
    m[3] = m3; m[4] = m4; m[5] = cy - (m3 * hx + m4 * hy);
}

extern "C" int lh_roi_affine(const float* boxes_dev, const float* rot_dev, const int* mirror_dev, const int* frame_index_dev, int b,
                             int n_frames, int h, int w, float padding, float* mat_dev, int* src_frame_dev, void* stream) {
    LH_REQUIRE(boxes_dev && rot_dev && mirror_dev && frame_index_dev && mat_dev && src_frame_dev && b > 0 && n_frames > 0 && h > 0 && w > 0
               && padding > 0.f && padding <= 3.0e38f, "lh_roi_affine: bad arguments");
    hipLaunchKernelGGL(roi_affine_kernel, dim3((b + 63) / 64), dim3(64), 0, (hipStream_t)stream, boxes_dev, rot_dev, mirror_dev,
                       frame_index_dev, b, n_frames, (float)h, (float)w, padding, mat_dev, src_frame_dev);
    LH_LAUNCH_CHECK("roi_affine launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ keypoints -> next oriented ROI
// The oriented sibling of keypoints_to_boxes_kernel.  The hand's up direction u is the unit vector from joint axis_from to joint
// axis_to when both are confident and at least min_axis apart; the crop's -y axis must point along it, so the crop's +x axis is
// (-u.y, u.x), with or without mirroring.  Otherwise the incoming direction is kept (normalised).  The confident joints are bounded
// along that direction and its normal; the box is those extents about the centre taken back to the frame.
__global__ void keypoints_to_rois_kernel(const float* preds, const float* maxvals, const float* boxes, const float* rot, const int* src_frame,
                                         int b, int j, int axis_from, int axis_to, float min_score, int min_joints, float min_side,
                                         float min_axis, float* next_boxes, float* next_rot, int* lost) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b) return;
    const float* p = preds + (long)i * j * 2;
    const float* mv = maxvals + (long)i * j;
    const float rx = rot[i * 2], ry = rot[i * 2 + 1];
    const float rn = sqrtf(rx * rx + ry * ry);
    float c = rx / rn, s = ry / rn;
    if (mv[axis_from] >= min_score && mv[axis_to] >= min_score) {
        const float dx = p[axis_to * 2] - p[axis_from * 2], dy = p[axis_to * 2 + 1] - p[axis_from * 2 + 1];
        const float d = sqrtf(dx * dx + dy * dy);
        if (d >= min_axis) { c = -(dy / d); s = dx / d; }
    }
    float lo_p = 0.f, lo_q = 0.f, hi_p = 0.f, hi_q = 0.f;
    int n = 0;
    for (int k = 0; k < j; ++k) {
        if (!(mv[k] >= min_score)) continue;
        const float x = p[k * 2], y = p[k * 2 + 1];
        const float u = x * c + y * s, v = y * c - x * s;
        if (n == 0) { lo_p = hi_p = u; lo_q = hi_q = v; }
        lo_p = u < lo_p ? u : lo_p; hi_p = u > hi_p ? u : hi_p;
        lo_q = v < lo_q ? v : lo_q; hi_q = v > hi_q ? v : hi_q;
        ++n;
    }
    float* o = next_boxes + i * 4;
    if (n < min_joints || src_frame[i] < 0 || !(isfinite(c) && isfinite(s))) {      // lost, empty, or no direction at all: keep the ROI
        o[0] = boxes[i * 4]; o[1] = boxes[i * 4 + 1]; o[2] = boxes[i * 4 + 2]; o[3] = boxes[i * 4 + 3];
        next_rot[i * 2] = rx; next_rot[i * 2 + 1] = ry;
        lost[i] = 1;
        return;
    }
    if (hi_p - lo_p < min_side) { const float m = (lo_p + hi_p) * 0.5f; lo_p = m - min_side * 0.5f; hi_p = m + min_side * 0.5f; }
    if (hi_q - lo_q < min_side) { const float m = (lo_q + hi_q) * 0.5f; lo_q = m - min_side * 0.5f; hi_q = m + min_side * 0.5f; }
    const float cp = (lo_p + hi_p) * 0.5f, cq = (lo_q + hi_q) * 0.5f, hp = (hi_p - lo_p) * 0.5f, hq = (hi_q - lo_q) * 0.5f;
    const float fx = cp * c - cq * s, fy = cp * s + cq * c;
    o[0] = fx - hp; o[1] = fy - hq; o[2] = fx + hp; o[3] = fy + hq;
    next_rot[i * 2] = c; next_rot[i * 2 + 1] = s;
    lost[i] = 0;
}

extern "C" int lh_keypoints_to_rois(const float* preds_dev, const float* maxvals_dev, const float* boxes_dev, const float* rot_dev,
                                    const int* src_frame_dev, int b, int j, int axis_from, int axis_to, float min_score, int min_joints,
                                    float min_side, float min_axis, float* next_boxes_dev, float* next_rot_dev, int* lost_dev, void* stream) {
    LH_REQUIRE(preds_dev && maxvals_dev && boxes_dev && rot_dev && src_frame_dev && next_boxes_dev && next_rot_dev && lost_dev && b > 0 && j > 0
               && min_joints >= 1 && (long)b * j < (1L << 30) && min_side >= 0.f && min_side <= 3.0e38f && min_score == min_score
               && min_axis > 0.f && min_axis <= 3.0e38f && axis_from >= 0 && axis_from < j && axis_to >= 0 && axis_to < j && axis_from != axis_to
               && next_boxes_dev != boxes_dev && next_rot_dev != rot_dev, "lh_keypoints_to_rois: bad arguments");
    hipLaunchKernelGGL(keypoints_to_rois_kernel, dim3((b + 63) / 64), dim3(64), 0, (hipStream_t)stream, preds_dev, maxvals_dev, boxes_dev,
                       rot_dev, src_frame_dev, b, j, axis_from, axis_to, min_score, min_joints, min_side, min_axis, next_boxes_dev,
                       next_rot_dev, lost_dev);
    LH_LAUNCH_CHECK("keypoints_to_rois launch");
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ One-Euro filter (Casiez et al. 2012)
// One workgroup per slot, one thread per coordinate (strided when j * 2 > 64).  init is per slot: every thread reads it before the
// barrier, thread 0 writes it after.  A slot that is empty or lost passes x through, leaves xhat / dxhat alone and ends with init = 0,
// so the hand starts fresh when it is found again.
__global__ __launch_bounds__(64) void one_euro_kernel(const float* x_in, const int* src_frame, const int* lost, const float* dt_in, int j2,
                                                      float min_cutoff, float beta, float d_cutoff, float* xhat, float* dxhat, int* init,
                                                      float* out) {
    const int slot = blockIdx.x;
    const bool away = src_frame[slot] < 0 || (lost && lost[slot] != 0);
    const float dt = dt_in[slot];
    const bool fresh = init[slot] == 0 || !(dt > 0.f) || !isfinite(dt);
    const float rd = (6.2831855f * d_cutoff) * dt, ad = rd / (rd + 1.f);
    for (int k = threadIdx.x; k < j2; k += blockDim.x) {
        const long e = (long)slot * j2 + k;
        const float x = x_in[e];
        if (away) { out[e] = x; continue; }
        if (fresh) { xhat[e] = x; dxhat[e] = 0.f; out[e] = x; continue; }
        const float xh = xhat[e];
        const float dx = (x - xh) / dt;
        const float dxh = ad * dx + (1.f - ad) * dxhat[e];
        const float fc = min_cutoff + beta * fabsf(dxh);
        const float r = (6.2831855f * fc) * dt, al = r / (r + 1.f);
        const float nx = al * x + (1.f - al) * xh;
        dxhat[e] = dxh; xhat[e] = nx; out[e] = nx;
    }
    __syncthreads();
    if (threadIdx.x == 0) init[slot] = away ? 0 : 1;
}

extern "C" int lh_one_euro(const float* x_dev, const int* src_frame_dev, const int* lost_dev, const float* dt_dev, int b, int j,
                           float min_cutoff, float beta, float d_cutoff, float* xhat_dev, float* dxhat_dev, int* init_dev, float* out_dev,
                           void* stream) {
    LH_REQUIRE(x_dev && src_frame_dev && dt_dev && xhat_dev && dxhat_dev && init_dev && out_dev && b > 0 && j > 0 && (long)b * j < (1L << 30)
               && min_cutoff > 0.f && min_cutoff <= 3.0e38f && beta >= 0.f && beta <= 3.0e38f && d_cutoff > 0.f && d_cutoff <= 3.0e38f
               && xhat_dev != x_dev && dxhat_dev != x_dev && xhat_dev != dxhat_dev && out_dev != xhat_dev && out_dev != dxhat_dev,
               "lh_one_euro: bad arguments");
    hipLaunchKernelGGL(one_euro_kernel, dim3(b), dim3(64), 0, (hipStream_t)stream, x_dev, src_frame_dev, lost_dev, dt_dev, j * 2, min_cutoff,
                       beta, d_cutoff, xhat_dev, dxhat_dev, init_dev, out_dev);
    LH_LAUNCH_CHECK("one_euro launch");
    return LH_OK;
}
