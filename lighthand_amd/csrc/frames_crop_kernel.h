// Device side of the frame crop (frames_crop.hip): the crop of a shared uint8 frame buffer -- or of decoder surfaces -- to padded NHWC4
// through one crop matrix per slot (roi_track.hip writes them).  CropArgs, the sample function of each frame format, the pixel loops, the
// two small modes of training on frames, and frames_crop_kernel itself.  Every rule stands above the code that implements it.
// Coordinates are pixel indices (pixel centres on the integers, an image spans [-0.5, size-0.5]).
// All arithmetic is fp32 in the order written (-ffp-contract=off): lighthand_amd/topdown.py restates it in numpy.
#pragma once
#include "common.h"
#include "color_jitter.h"
#include "tracks_manage_kernel.h"
#include "motion_kernel.h"

// ------------------------------------------------------------------------------------------------ frames -> crops
// Slot blockIdx.y reads frame src_frame[slot] of a buffer every slot shares: several boxes per frame, frames of any size.  The slot's
// matrix and frame number are the same for the whole workgroup (scalar loads); one thread per pixel of the padded output, as
// image_u8_kernel.  A gather over bytes: neighbouring lanes read neighbouring source pixels (a box maps rows to rows), the four taps
// of a pixel share cache lines with its neighbours', and the frame's reuse across the boxes that read it is the L2's.
enum { LH_FRAMES_RGB = 0, LH_FRAMES_NV12 = 1, LH_FRAMES_420 = 2, LH_FRAMES_420W = 3 };
#include "draw_hands_kernel.h"                                    // (behind the format codes: it draws through them)

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
    // ColorJitter (the rule: in frames_crop_kernel, above its two modes): null = none, and the crop entries without it read none of the three
    const float* jfactors;                                        // [b][4] brightness, contrast, saturation, hue
    const int* jorder;                                            // [b][4] op ids, negative = skip
    double* jpartial;                                             // [b][CJ_STRIPS]: written by LH_CROP_GREY_MEAN, read by the apply mode
    int jdtype;                                                   // the apply mode: the dtype of dst (the launch is the fp32 instantiation's)
    // lh_frames_crop_surfaces_to_nhwc4 (the rules: above crop_texel and above the table load in frames_crop_kernel; gen = 0: none of it is
    // read).  The fp32 instantiation's, stores in jdtype.
    int gen;
    const long long* table;                                       // [n_frames] device addresses (0 = empty), or null: src + f * frame_stride
    int dsc[4];                                                   // LH_FRAMES_420 / 420W: c_pitch, cb_offset, cr_offset, c_step (with pitch, siting)
    TracksArgs tm;                                                // op = LH_CROP_TRACKS_MANAGE (lh_tracks_manage, tracks_manage_kernel.h): all it reads
    PredictArgs pr;                                               // op = LH_CROP_ROIS_PREDICT (lh_rois_predict, motion_kernel.h): all it reads
    GatedArgs og;                                                 // op = LH_CROP_ONE_EURO_GATED (lh_one_euro_gated, motion_kernel.h): all it reads
    DrawArgs dr;                                                  // op = LH_CROP_DRAW_HANDS (lh_draw_hands, draw_hands_kernel.h): beside the fields it names
};
// frames_crop.hip: a launch of the fp32 instantiation with `grid` workgroups of `block` threads and `lds` bytes of dynamic LDS, for an
// entry in another file (tracks_manage.hip, motion.hip, draw_hands.hip); the caller runs LH_LAUNCH_CHECK.
void lh_frames_crop_launch_f32(const CropArgs& a, int grid, int block, size_t lds, void* stream);
// frames_crop.hip: the checks of a plane descriptor and the fields of ``a`` a kernel finds its samples through (lh_draw_hands shares them)
int lh_frames_layout_args(const char* who, const lh_frames_layout* layout, int hs, int ws, const unsigned char* frames, long frame_stride,
                          CropArgs& a);
enum { LH_CROP = 0, LH_CROP_ROI_PERTURB = 1, LH_CROP_POINTS_INV = 2, LH_CROP_GREY_MEAN = 3, LH_CROP_TRACKS_MANAGE = 4, LH_CROP_ROIS_PREDICT = 5,
       LH_CROP_ONE_EURO_GATED = 6, LH_CROP_DRAW_HANDS = 7 };
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

// ------------------------------------------------------------------------------------------------ one sample, per frame format
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
// base is the frame's first luma byte.  One frame's bytes are a 32-bit quantity (frame_stride < 2^31).
// csc = k[9], o[3] in VECTOR registers (crop_slot).
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

// The other 4:2:0 flavours (lh_frames_crop_surfaces_to_nhwc4): where a sample's bytes are.  One plane descriptor (format =
// LH_FRAMES_420, or LH_FRAMES_420W for 16-bit samples) covers NV12, NV21, planar yuv420p and 10-bit P010: luma sample (x, y) at
// y*pitch + x*sample_bytes, Cb / Cr of chroma sample (cx, cy) at cb_offset / cr_offset + cy*c_pitch + cx*c_step.  A 16-bit sample is
// little-endian and its texel value is (float)(u16 >> 6) * 0.25f -- the 10 significant bits on the 8-bit scale, exact in fp32, the low
// 6 bits never data.  Everything after the texel fetch is the NV12 rule above, in the same order (crop_sample_420 is crop_sample_nv12
// with the descriptor's addresses), so NV12 through the descriptor gives lh_frames_crop_yuv_to_nhwc4's bits.  The sample width picks
// the body in front of the pixel loops, as format does.  All of it is the fp32 instantiation's (gen != 0), which then stores in jdtype
// as the ColorJitter apply mode does: the 16-bit instantiations carry none of it.  topdown.py: frames_crop_yuv420_host.
// U = unsigned char: 8-bit samples; unsigned short: P010's.  Offsets are 32-bit (a frame is below 2^31 bytes).
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

// ------------------------------------------------------------------------------------------------ the pixels of one slot
// Area sampling of minified ROIs (lh_frames_crop_area_to_nhwc4; max_taps = 1 is the plain crop).  One bilinear sample per crop pixel
// skips frame pixels as soon as a crop pixel covers more than one of them, so a minified crop averages kx x ky samples spread evenly
// over each crop pixel's footprint instead.  The rule, fp32 in this order; topdown.py's frames_crop_host / crop_taps_host restate it.
// Per slot, from its matrix (crop_taps):
//     sx = sqrtf(m0*m0 + m3*m3), sy = sqrtf(m1*m1 + m4*m4)          frame pixels per crop pixel along the crop's x and y axes
//     kx = sx > 1.015625f && isfinite(sx) ? min(max_taps, (int)ceilf(fminf(sx, 64.f))) : 1, ky likewise from sy
// A NaN scale fails the comparison and gives 1, an infinite one is given 1 (such a matrix puts every sample outside the frame); the
// 1/64 slack keeps a ROI at scale 1 + rounding error on the single-sample path.
// Per output pixel (ox, oy), j = 0..ky-1 outside and i = 0..kx-1 inside (crop_pixels):
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
__device__ __forceinline__ int crop_taps(float a, float b, int max_taps) {
    const float s = sqrtf(a * a + b * b);
    return s > 1.015625f && isfinite(s) ? min(max_taps, (int)ceilf(fminf(s, 64.f))) : 1;
}

// FMT (LH_FRAMES_*) picks the sample function, nothing else: the walk, the tap offsets, the accumulation and the store are shared.
template <int FMT>
__device__ __forceinline__ bool crop_sample_of(const CropArgs& p, const float* csc, const unsigned char* base, float fx, float fy, float s[3]) {
    if constexpr (FMT == LH_FRAMES_420) return crop_sample_420<unsigned char>(p, csc, base, fx, fy, s);
    else if constexpr (FMT == LH_FRAMES_420W) return crop_sample_420<unsigned short>(p, csc, base, fx, fy, s);
    else if constexpr (FMT == LH_FRAMES_NV12) return crop_sample_nv12(p, csc, base, fx, fy, s);
    else return crop_sample(base, p.hs, p.ws, fx, fy, s);
}

// The pixels of one slot.  AREA = false is the plain crop, one sample at the pixel's centre: the loop the kernel always had, kept apart
// from the tap loops so that it compiles to what it was.  AREA = true: a live slot, kx x ky samples over the pixel's footprint.
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

// ================================================================================================ the modes of training on frames
// lh_roi_perturb and lh_affine_points_inv (frames_crop.hip) launch frames_crop_kernel<float> with op != LH_CROP: one thread per slot or
// per point, nothing of the crop above is read.

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

// ================================================================================================ the kernel
template <typename T>
__global__ __launch_bounds__(256) void frames_crop_kernel(const CropArgs p) {
    if constexpr (sizeof(T) == 4) {                               // the fp32 instantiation alone carries the modes (CropArgs)
        // one branch for the four thread-per-item modes and the overlay: with a test of their own in front of the crop the two of motion_kernel.h took this
        // instantiation from 71 to 85 vector registers (7 waves a SIMD to 6); behind this one it allocates what it did
        if (p.op == LH_CROP_ROI_PERTURB || p.op == LH_CROP_POINTS_INV || p.op >= LH_CROP_ROIS_PREDICT) {
            if (p.op == LH_CROP_ROIS_PREDICT) rois_predict_slot(p.pr);               // grid (b / 64), 64 threads: lh_rois_predict's launch alone
            else if (p.op == LH_CROP_ONE_EURO_GATED) one_euro_gated_slot(p.og);      // grid (b), 64 threads: lh_one_euro_gated's launch alone
            else if (p.op == LH_CROP_DRAW_HANDS) {                                   // grid (b * DRAW_WGS), 256 threads, dynamic LDS: lh_draw_hands' launch alone
                extern __shared__ __attribute__((aligned(16))) unsigned char tm_lds[];
                draw_hands_slot(p, tm_lds);
            }
            else crop_aux_modes(p);
            return;
        }
        if (p.op == LH_CROP_TRACKS_MANAGE) {                      // grid (n_frames), 64 threads, dynamic LDS: lh_tracks_manage's launch alone
            extern __shared__ __attribute__((aligned(16))) unsigned char tm_lds[];
            tracks_manage_frame(p.tm, tm_lds);
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
        // Decoder surfaces (lh_frames_crop_surfaces_to_nhwc4).  The frame source is the buffer above (frame f at byte f * frame_stride) or
        // a SURFACE TABLE, int64 [n_frames] in device memory: entry f is the device address of frame f, read at every launch -- the
        // surfaces of a captured graph change with no recapture.  The entry is a scalar load (the slot is blockIdx.y) and is tested
        // before any address is formed from it: 0 is an empty frame, the slot's crop is black as an empty slot's.
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
        // ColorJitter on the crop (lh_frames_crop_jitter_to_nhwc4, training on frames): the uint8 input kernels' rule (color_jitter.h) on
        // the pixel's c[3] in 0..1 -- after the single sample, the tap average or the YUV conversion -- in the slot's op order, before
        // Normalize.  Two launches of this kernel.  The grey-mean mode (op = LH_CROP_GREY_MEAN, the fp32 instantiation whatever the
        // crop's dtype: the samples are fp32 in all three) walks the slot's interior through the crop's own sample path (the same kx, ky,
        // the same walk), applies the ops that precede contrast and reduces cj_gray in fp64: per thread in walk order, then a fixed tree
        // in LDS, one partial per workgroup into workspace[slot][CJ_STRIPS] (grid (CJ_STRIPS, b), no atomics: a replay is
        // bit-reproducible).  Pixels that fell outside the frame are black and count, as the warped uint8 path counts its black fill.  A
        // slot without a contrast op writes zeros and samples nothing.  The apply mode (op = LH_CROP with jfactors != null, a
        // workgroup-uniform switch in front of the pixel loops as format is; also the fp32 instantiation's, which then stores in jdtype:
        // the 16-bit instantiations carry no jitter code at all) sums the slot's partials in index order once per workgroup, mean =
        // (float)(sum / (h*w)), and runs cj_apply(c, factors, order, 0, 4, mean) between the sample and Normalize.  Order (-1, -1, -1, -1)
        // touches nothing: the un-jittered crop bit for bit.  An empty slot stays black: every op maps black with mean 0 to black.
        // topdown.py: frames_crop_jitter_host.
        // Both launches are this instantiation's, whatever the crop's dtype -- the samples are fp32 in all three, only the
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
