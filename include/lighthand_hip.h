/*
 * lighthand_hip.h -- C ABI of liblighthand_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the heatmap-regression hot path of leejeongho3214/LightHand.
 * The reference has no FFI of its own: all arithmetic on this
 * path is done by PyTorch/cuDNN underneath plain Python callables.  Each entry point
 * below therefore cites the reference call site whose device work it replaces
 * (paths relative to the reference root); the Python mirror of those callables lives
 * in lighthand_amd/ and reaches this library through ctypes (lighthand_amd/_lib.py).
 *
 * Conventions
 *  - the caller owns every buffer (device pointers unless stated); the library never
 *    allocates, frees or retains device memory;
 *  - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*);
 *    no entry point synchronises, so every call is legal inside hipGraph capture;
 *  - return 0 on success, a negative lh_status otherwise; lh_last_error() gives text;
 *  - activations are NHWC, `dtype` selects their element type (weights packs use the
 *    same type; BatchNorm vectors, loss, gradients of weights and Adam state are fp32);
 *  - weight tensors at the boundary keep the reference/PyTorch layouts (OIHW for
 *    Conv2d, [C_in, C_out, kH, kW] for ConvTranspose2d); the pack functions build the
 *    device-side K-major images the MFMA kernels consume.
 */
#ifndef LIGHTHAND_HIP_H
#define LIGHTHAND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { LH_F32 = 0, LH_BF16 = 1, LH_F16 = 2 } lh_dtype;

typedef enum {
    LH_OK = 0,
    LH_ERR_ARG = -1,      /* bad shape / dtype / alignment */
    LH_ERR_HIP = -2,      /* a HIP runtime call failed     */
    LH_ERR_UNSUPPORTED = -3
} lh_status;

int lh_version(void);
const char* lh_last_error(void);
/* number of bytes of one activation element for `dtype` */
int lh_dtype_size(int dtype);

/* ------------------------------------------------------------------ layout transforms
 * images.cuda() -> model(images): src/utils/method.py:165-167.  NCHW fp32 image batch ->
 * zero-padded NHWC4 image in the run dtype ([N][H+2*pad][Wp][4], channel 3 = 0), the
 * input format of the stem convolution kernel. */
int lh_image_to_nhwc4(const float* nchw, void* out, int n, int h, int w, int pad, int wp,
                      int dtype, void* stream);
/* Fused input pipeline (the CPU DataLoader work of src/tools/dataset.py:128-159 moved onto the device): uint8 HWC
 * [n][hs][ws][3] -> /255 -> bilinear resize to h x w (half-pixel centres, no antialias) -> (x - mean)/std (HOST
 * float[3] arrays) -> zero-padded NHWC4 in the run dtype, i.e. the stem's input format. */
int lh_image_u8_to_nhwc4(const unsigned char* hwc, void* out, int n, int hs, int ws, int h, int w, int pad, int wp,
                         const float* mean3, const float* std3, int dtype, void* stream);
/* The same with torchvision's ColorJitter(brightness, contrast, saturation, hue) between Resize and Normalize -- the
 * training transform of src/tools/dataset.py:134-146.  The random draw (ColorJitter.get_params) stays with the caller:
 * factors_dev fp32 [n][4] = per-image brightness / contrast / saturation / hue factors, order_dev int32 [n][4] = the op
 * order (op ids 0..3, a negative id skips: the reference jitters only a fraction of its samples).  workspace (device,
 * lh_image_jitter_workspace_bytes(n)) holds the fp64 strip sums of the per-image grey mean the contrast op needs. */
size_t lh_image_jitter_workspace_bytes(int n);
int lh_image_u8_jitter_to_nhwc4(const unsigned char* hwc, void* out, int n, int hs, int ws, int h, int w, int pad, int wp,
                                const float* mean3, const float* std3, const float* factors_dev, const int* order_dev,
                                void* workspace, int dtype, void* stream);
/* uint8 HWC -> per-image affine warp (inv_dev fp32 [n][6], output pixel-index coordinates, black outside the frame)
 * -> bilinear resize -> [ColorJitter when factors_dev != NULL] -> Normalize -> padded NHWC4 in the run dtype.
 * Output pixel (ox, oy) samples the resized frame at u = (a ox + b oy + c, d ox + e oy + f), inv = [a b c d e f]: inside
 * [-0.5, w-0.5] x [-0.5, h-0.5] with the resize rule above, outside as 0 (cv2.warpAffine's constant border); the
 * identity reproduces lh_image_u8_to_nhwc4 / lh_image_u8_jitter_to_nhwc4 bit for bit.  The contrast op's grey mean is that
 * of the warped image.  workspace: lh_image_jitter_workspace_bytes(n), unused (may be NULL) without jitter. */
int lh_image_u8_warp_to_nhwc4(const unsigned char* hwc, void* out, int n, int hs, int ws, int h, int w, int pad, int wp,
                              const float* mean3, const float* std3, const float* inv_dev,
                              const float* factors_dev, const int* order_dev, void* workspace, int dtype, void* stream);
/* points fp32 [b][j][pstride] -> out fp32 [b][j][ostride]: (x, y) through the forward matrix fwd_dev fp32 [b][6].  Points
 * that leave the frame are kept; out may alias pts when the strides agree. */
int lh_affine_points(const float* pts, int pstride, const float* fwd_dev, float* out, int ostride, int b, int j, void* stream);
/* Flip test: mirror the w interior pixels of every row of a padded NHWC4 image [n][h+2*pad][wp][4] (the layout
 * lh_image_to_nhwc4 and the lh_image_u8_* entries write, run dtype) in place, img'[y][x] = img[y][w-1-x]; the padding is
 * not touched.  A bit-exact copy: a second call restores the input. */
int lh_nhwc4_mirror(void* img, int n, int h, int w, int pad, int wp, int dtype, void* stream);
/* Top-down inference on full frames.  Coordinates are pixel indices (pixel centres on the integers, an image spans
 * [-0.5, size-0.5]); a box is (x0, y0, x1, y1), the box that encloses pixels i0..i1 is (i0-0.5, i1+0.5).  All fp32, in this order:
 * lh_box_affine: boxes_dev fp32 [b][4], frame_index_dev int32 [b] -> mat_dev fp32 [b][6] (crop pixel index -> frame pixel index of
 * an h x w crop) and src_frame_dev int32 [b].  bw = x1-x0, bh = y1-y0, cx = (x0+x1)*0.5, cy = (y0+y1)*0.5,
 * sw = padding * max(bw, bh*w/h), sh = sw*h/w, a = sw/w, mat = [a, 0, (cx - sw*0.5) + a*0.5, 0, a, (cy - sh*0.5) + a*0.5].
 * src_frame[i] = frame_index[i] when that lies in 0..n_frames-1 and the box is finite with bw > 0 and bh > 0; otherwise the slot
 * is empty: src_frame[i] = -1 and mat[i] = 0. */
int lh_box_affine(const float* boxes_dev, const int* frame_index_dev, int b, int n_frames, int h, int w, float padding,
                  float* mat_dev, int* src_frame_dev, void* stream);
/* frames_u8 [n_frames][hs][ws][3], shared by all b slots -> padded NHWC4 crops [b][h+2*pad][wp][4] in the run dtype.  Output pixel
 * (ox, oy) of slot i samples frame src_frame[i] at fx = (m0*ox + m1*oy) + m2, fy = (m3*ox + m4*oy) + m5: inside
 * [-0.5, ws-0.5] x [-0.5, hs-0.5] bilinearly with lh_image_u8_warp_to_nhwc4's edge clamp and blend order, * (1/255); outside
 * (NaN included) and in every pixel of an empty slot (src_frame outside 0..n_frames-1) black, 0 before Normalize; then
 * (c - mean) * (1/std) (HOST float[3] arrays).  The whole buffer is written: padding and channel 3 are zero.  out must be 8-byte aligned
 * (every dtype: the 16-bit dtypes store a pixel record as one 8-byte word).  A whole-frame box
 * with hs = h, ws = w and padding 1 reproduces lh_image_u8_to_nhwc4 bit for bit. */
int lh_frames_crop_to_nhwc4(const unsigned char* frames_u8, void* out, int b, int n_frames, int hs, int ws, int h, int w, int pad,
                            int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                            int dtype, void* stream);
/* The antialiased sibling (opt-in; the same kernel, and max_taps = 1 is lh_frames_crop_to_nhwc4 bit for bit): a minified ROI averages
 * kx x ky of the samples above, spread evenly over each crop pixel's footprint.  fp32, in this order.  Per slot:
 * sx = sqrtf(m0*m0 + m3*m3), sy = sqrtf(m1*m1 + m4*m4) (frame pixels per crop pixel along the crop's axes),
 * kx = sx > 1.015625f && isfinite(sx) ? min(max_taps, (int)ceilf(fminf(sx, 64.f))) : 1, ky likewise from sy (a NaN or infinite
 * scale gives 1: every sample of such a slot is outside the frame; a slot that is not minified takes the single sample).  Per
 * output pixel, j = 0..ky-1 outside, i = 0..kx-1 inside: dy = (float)(2*j + 1 - ky) / (float)(2*ky) (= (j + 0.5) / ky - 0.5, rounded
 * once), uy = (float)oy + dy, dx and ux likewise, fx = (m0*ux + m1*uy) + m2, fy = (m3*ux + m4*uy) + m5, acc[ch] += the sample at
 * (fx, fy) on the raw 0..255 values (same inside test, clamp and blend; outside or NaN adds 0); then
 * c = (acc * (1.f / (float)(kx*ky))) * (1/255) and Normalize as above.  An aligned integer minification s = 2, 3, 4, 6 or 8
 * <= max_taps (m = (s, 0, (s-1)/2, 0, s, (s-1)/2)) is the exact mean of each s x s block, bit for bit, for crops up to 512 pixels
 * a side; above max_taps the taps are more than one frame pixel apart (aliasing reduced, not removed).
 * max_taps outside 1..8 is LH_ERR_ARG. */
int lh_frames_crop_area_to_nhwc4(const unsigned char* frames_u8, void* out, int b, int n_frames, int hs, int ws, int h, int w, int pad,
                                 int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                                 int max_taps, int dtype, void* stream);
/* The NV12 sibling (opt-in; the same kernel, the two entries above keep their output bits): the frames are what a video decoder
 * writes, 8-bit 4:2:0 with interleaved chroma, and the colour conversion runs per sample on the ROI only.  Frame f starts at byte
 * f * frame_stride of frames_nv12; luma byte (x, y) is at y*pitch + x; Cb and Cr of chroma sample (cx, cy) are at
 * uv_offset + cy*pitch + 2*cx and that address + 1; wc = ws/2, hc = hs/2.  The tight layout is pitch = ws, uv_offset = hs*ws,
 * frame_stride = hs*ws*3/2; a decoder surface has pitch >= ws and uv_offset = pitch * aligned_height.  csc12 is a HOST float[12]
 * copied by value: k[3][3] row-major, then o[3].  max_taps 1..8 as lh_frames_crop_area_to_nhwc4's (1: the plain crop).  Every sample
 * at (fx, fy) -- the pixel's centre or one tap of the area rule -- fp32, in this order: the inside test and the lower clamp to 0 of
 * the RGB entries give (cx_, cy_); Y is their bilinear sample of one channel on the luma plane (same indices, upper index clamp,
 * weights wx, wy and blend top + (bot - top) * wy); gx = chroma_siting == 0 ? cx_ * 0.5f : (cx_ - 0.5f) * 0.5f,
 * gy = (cy_ - 0.5f) * 0.5f (siting 0, "left": chroma co-sited with the even luma columns, the H.264 / HEVC default; 1, "center":
 * between them, JPEG / MPEG-1; vertically centred in both), gx = fminf(fmaxf(gx, 0), wc-1), gy = fminf(fmaxf(gy, 0), hc-1); U and V
 * are the same blend on the chroma plane at (gx, gy) with x0 = min((int)gx, wc-1), x1 = min(x0+1, wc-1) and y likewise;
 * e0 = Y - o[0], e1 = U - o[1], e2 = V - o[2], s[c] = fminf(fmaxf((k[c][0]*e0 + k[c][1]*e1) + k[c][2]*e2, 0.f), 255.f).  s is then
 * the RGB entries' sample: * (1/255) or the tap sum and (acc * inv) * (1/255), Normalize, the store; a sample outside the frame or
 * NaN, an empty slot (which never forms an address), padding and channel 3 behave as there.  Frames with CbCr = 128 and k[c][0] = 1,
 * o[0] = 0 give the RGB entries' bits on the grey frames.  LH_ERR_ARG, before any device work: hs, ws odd or < 2; pitch < ws;
 * uv_offset < pitch*hs; uv_offset + (hc-1)*pitch + ws > frame_stride; frame_stride >= 2^31; chroma_siting outside {0, 1}; a
 * coefficient that is not finite; max_taps, dtype and alignment as above. */
int lh_frames_crop_yuv_to_nhwc4(const unsigned char* frames_nv12, void* out, int b, int n_frames, int hs, int ws, int pitch,
                                int uv_offset, long frame_stride, int chroma_siting, const float* csc12, int h, int w, int pad, int wp,
                                const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev, int max_taps,
                                int dtype, void* stream);
/* The frame crop with torchvision's ColorJitter between the sample and Normalize (training on frames: runtime.TrainStep(frames=...,
 * crop_jitter=...)): lh_frames_crop_yuv_to_nhwc4's arguments -- csc12 == NULL: packed RGB frames as lh_frames_crop_area_to_nhwc4 reads
 * them, and pitch, uv_offset, frame_stride and chroma_siting are not looked at -- plus factors_dev fp32 [b][4] (brightness, contrast,
 * saturation, hue), order_dev int32 [b][4] (op ids 0..3, a negative id skips) and workspace (device, 8-byte aligned,
 * lh_frames_crop_jitter_workspace_bytes(b)): lh_image_u8_jitter_to_nhwc4's draw, per slot.  The rule is that kernel's, on the crop:
 * the ops run in the slot's order on the pixel's three channels in 0..1 (after the single sample, the tap average or the YUV
 * conversion) and Normalize follows.  Contrast blends with the grey mean of the slot's whole h x w crop as it stands when the op runs;
 * pixels that fell outside the frame are black and count.  Two launches: the first reduces each slot's grey sum into 32 fp64 partials
 * (fixed order, no atomics: a replay is bit-reproducible; a slot without a contrast op writes zeros and samples nothing), the second
 * sums them in index order, mean = (float)(sum / (h*w)), and writes the crop.  A slot whose order is (-1, -1, -1, -1) is the
 * un-jittered entry's crop bit for bit; an empty slot stays black.  LH_ERR_ARG: factors_dev, order_dev or workspace NULL, and
 * everything the entry it extends refuses. */
size_t lh_frames_crop_jitter_workspace_bytes(int b);
int lh_frames_crop_jitter_to_nhwc4(const unsigned char* frames, void* out, int b, int n_frames, int hs, int ws, int pitch, int uv_offset,
                                   long frame_stride, int chroma_siting, const float* csc12, int h, int w, int pad, int wp,
                                   const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev, int max_taps,
                                   const float* factors_dev, const int* order_dev, void* workspace, int dtype, void* stream);
/* Decoder surfaces read in place, and the other 4:2:0 flavours (opt-in; the same kernel, the entries above keep their arguments,
 * checks and output bits).  The frame source is EITHER frames with frame_stride (frame f starts at byte f * frame_stride, as
 * lh_frames_crop_yuv_to_nhwc4's buffer) OR surface_table_dev, int64 [n_frames] in device memory, 8-byte aligned: entry f is the device
 * address of frame f.  The table is read by the launch, so a captured graph follows a rebound table with no recapture; an entry of 0
 * is an empty frame -- it is tested before any address is formed, and the slot's crop is black as an empty slot's.  Exactly one of
 * the two is non-NULL.  layout (HOST, copied by value) says where a sample's bytes are, from the frame's first byte:
 *   format LH_FRAMES_FMT_RGB      packed [hs][ws][3]; nothing else of the struct is read
 *          LH_FRAMES_FMT_NV12     luma (x, y) at y*pitch + x;    Cb of chroma sample (cx, cy) at cb_offset + cy*c_pitch + 2*cx, Cr = Cb + 1
 *          LH_FRAMES_FMT_NV21     luma as nv12;                  Cr at cr_offset + cy*c_pitch + 2*cx, Cb = Cr + 1
 *          LH_FRAMES_FMT_YUV420P  luma y*pitch + x;              Cb at cb_offset + cy*c_pitch + cx, Cr at cr_offset + cy*c_pitch + cx
 *                                 (cr_offset below cb_offset is YV12)
 *          LH_FRAMES_FMT_P010     luma y*pitch + 2*x;            Cb at cb_offset + cy*c_pitch + 4*cx, Cr = Cb + 2; samples are
 *                                 little-endian 16-bit and a texel's value is (float)(u16 >> 6) * 0.25f: the 10 significant bits on the
 *                                 8-bit scale, exact in fp32; the low 6 bits are never read as data
 * Everything after the texel fetch is lh_frames_crop_yuv_to_nhwc4's rule in its fp32 order (inside test, clamps, chroma position
 * from chroma_siting, the two blends, e = yuv - o, the 3 x 3 product, the clip) and from there the RGB entries' handling; NV12 input
 * gives that entry's bits.  factors_dev / order_dev / workspace: all NULL, or lh_frames_crop_jitter_to_nhwc4's triple (ColorJitter
 * between the sample and Normalize, its two launches).  Every launch is the fp32 instantiation's, which stores in dtype.
 * LH_ERR_ARG, before any launch: both sources NULL or both set; an unknown format; odd sides or sides < 2; pitch or c_pitch below a
 * row's bytes; a chroma plane that starts inside the luma plane; overlapping planar chroma planes; cb_offset / cr_offset not in the
 * format's relation; planes that end outside frame_bytes or at 2^31 or beyond; frame_stride below the bytes a frame's samples span;
 * an odd p010 pitch, c_pitch, offset, frames address or frame_stride; chroma_siting outside {0, 1}; a coefficient that is not
 * finite; and what the entries above refuse. */
enum { LH_FRAMES_FMT_RGB = 0, LH_FRAMES_FMT_NV12 = 1, LH_FRAMES_FMT_NV21 = 2, LH_FRAMES_FMT_YUV420P = 3, LH_FRAMES_FMT_P010 = 4 };
typedef struct lh_frames_layout {
    int format;                 /* LH_FRAMES_FMT_* */
    int pitch, c_pitch;         /* bytes between luma rows / between chroma rows */
    int cb_offset, cr_offset;   /* byte offsets of the first Cb and the first Cr sample */
    int frame_bytes;            /* the bytes of one frame: every plane ends inside them */
    int chroma_siting;          /* 0 left, 1 center */
    float csc12[12];            /* k[3][3] row-major, then o[3] */
} lh_frames_layout;
int lh_frames_crop_surfaces_to_nhwc4(const unsigned char* frames, void* out, long frame_stride, const long long* surface_table_dev,
                                     const lh_frames_layout* layout, int b, int n_frames, int hs, int ws, int h, int w, int pad,
                                     int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                                     int max_taps, const float* factors_dev, const int* order_dev, void* workspace, int dtype, void* stream);
/* preds_dev fp32 [b][j][2] (frame coordinates), maxvals_dev fp32 [b][j] -> next_boxes_dev fp32 [b][4], lost_dev int32 [b]: the bounds
 * of the keypoints with maxval >= min_score, each side widened about its centre to at least min_side.  With fewer than min_joints
 * such keypoints, or for an empty slot (src_frame < 0), next_boxes[i] = boxes[i] and lost[i] = 1; otherwise lost[i] = 0.  No
 * atomics: bit-reproducible.  next_boxes_dev must not be boxes_dev. */
int lh_keypoints_to_boxes(const float* preds_dev, const float* maxvals_dev, const float* boxes_dev, const int* src_frame_dev, int b,
                          int j, float min_score, int min_joints, float min_side, float* next_boxes_dev, int* lost_dev, void* stream);
/* Oriented, mirrored ROIs (opt-in siblings of the two entries above; the crop kernel and lh_affine_points take the matrix as it is).
 * lh_roi_affine: as lh_box_affine, plus rot_dev fp32 [b][2] = (rx, ry), the frame direction of the crop's +x axis (any length,
 * (1, 0) = upright) and mirror_dev int32 [b] (non-zero: the crop's x axis is flipped, a left hand reaches the network as a right
 * one).  The box gives the ROI's centre and its extents along the ROI's own axes (the box before it is turned about its centre).
 * bw, bh, cx, cy, sw, a as lh_box_affine's; n = sqrtf(rx*rx + ry*ry), c = rx/n, s = ry/n, ac = a*c, as = a*s, g = mirror ? -1 : 1,
 * m0 = g*ac, m1 = -as, m3 = g*as, m4 = ac, hx = (w-1)*0.5, hy = (h-1)*0.5, m2 = cx - (m0*hx + m1*hy), m5 = cy - (m3*hx + m4*hy).
 * Empty slots as lh_box_affine's, and also when rot is not finite or n is not > 0. */
int lh_roi_affine(const float* boxes_dev, const float* rot_dev, const int* mirror_dev, const int* frame_index_dev, int b, int n_frames,
                  int h, int w, float padding, float* mat_dev, int* src_frame_dev, void* stream);
/* The oriented sibling of lh_keypoints_to_boxes: next_boxes_dev fp32 [b][4], next_rot_dev fp32 [b][2], lost_dev int32 [b].  With
 * both anchor joints confident (maxval >= min_score) and d = sqrtf(dx*dx + dy*dy) >= min_axis, (dx, dy) = p[axis_to] - p[axis_from]:
 * (c, s) = next_rot = (-(dy/d), dx/d), so that the crop's -y axis points from axis_from to axis_to (mirrored or not); otherwise
 * (c, s) = rot / its norm.  Every confident joint is projected, p = x*c + y*s, q = y*c - x*s; their bounds, each widened about its
 * centre to at least min_side, give the centre (cp, cq) and half extents (hp, hq); the centre returns to the frame as
 * (cp*c - cq*s, cp*s + cq*c) and next_boxes = centre -+ half extents.  With fewer than min_joints confident joints, for an empty
 * slot (src_frame < 0) or when (c, s) is not finite, next_boxes = boxes, next_rot = rot and lost = 1.  One thread per slot, no
 * atomics.  min_axis > 0, axis_from != axis_to, both in 0..j-1; the outputs must not be boxes_dev / rot_dev. */
int lh_keypoints_to_rois(const float* preds_dev, const float* maxvals_dev, const float* boxes_dev, const float* rot_dev,
                         const int* src_frame_dev, int b, int j, int axis_from, int axis_to, float min_score, int min_joints,
                         float min_side, float min_axis, float* next_boxes_dev, float* next_rot_dev, int* lost_dev, void* stream);
/* One-Euro filter (Casiez et al. 2012) of x_dev fp32 [b][j][2] into out_dev, one launch per frame; state xhat_dev, dxhat_dev fp32
 * [b][j][2] and init_dev int32 [b]; dt_dev fp32 [b] in seconds; lost_dev int32 [b] may be NULL.  alpha(fc) = r / (r + 1) with
 * r = (6.2831855f * fc) * dt.  init[slot] = 1: dx = (x - xhat) / dt, ad = alpha(d_cutoff), dxhat = ad*dx + (1-ad)*dxhat,
 * fc = min_cutoff + beta*fabsf(dxhat), al = alpha(fc), xhat = al*x + (1-al)*xhat, out = xhat.  init[slot] = 0, or dt not finite or
 * not > 0: xhat = x, dxhat = 0, out = x.  init becomes 1.  A slot with src_frame < 0 or lost != 0 passes x through, keeps its state
 * and ends with init = 0.  One workgroup per slot; init is written behind a barrier.  min_cutoff, d_cutoff > 0, beta >= 0 (it
 * multiplies |dxhat|, units of x per second). */
int lh_one_euro(const float* x_dev, const int* src_frame_dev, const int* lost_dev, const float* dt_dev, int b, int j, float min_cutoff,
                float beta, float d_cutoff, float* xhat_dev, float* dxhat_dev, int* init_dev, float* out_dev, void* stream);
/* Track management of the tracked step (opt-in; runtime.ManagedInferStep(frames=..., track=True, manage_tracks=...)), one launch behind
 * lh_keypoints_to_boxes / lh_keypoints_to_rois and in front of lh_one_euro; it edits next_boxes_dev fp32 [b][4], next_rot_dev fp32
 * [b][2] (may be NULL: upright steps) and lost_dev int32 [b] in place and keeps lost_count_dev int32 [b] (state: frames a slot has been
 * lost).  Slot i belongs to frame f = frame_index[i] when 0 <= f < n_frames; any other slot is never touched, and frames are
 * independent.  The detection list has k entries: det_boxes_dev fp32 [k][4] = x0 y0 x1 y1 (frame pixel indices), det_frame_dev int32
 * [k], det_score_dev fp32 [k]; an entry is valid when its frame is in range, its coordinates are finite, x1 > x0, y1 > y0 and its
 * score is finite and >= det_min_score.  All arithmetic is fp32 in the order written, without division or sqrtf; min / max are
 * "a < b ? a : b" / "a > b ? a : b".
 *  1. kb[i] = the bounds lh_keypoints_to_boxes computes from preds_dev fp32 [b][j][2] / maxvals_dev fp32 [b][j]: min / max of the
 *     joints with maxval >= track_min_score in ascending order, each side widened about its centre to track_min_side (axis-aligned in
 *     the frame under oriented ROIs too); score[i] = the sum of those maxvals in ascending order.  A slot is live when lost[i] == 0.
 *  2. over(a, b, t): iw = min(ax1, bx1) - max(ax0, bx0), ih likewise; false unless iw > 0 && ih > 0; else
 *     iw*ih > t * min((ax1-ax0)*(ay1-ay0), (bx1-bx0)*(by1-by0)) -- intersection over the smaller area.
 *  3. The live slots of a frame are walked in descending score (ties: lower index); a slot is kept unless over(kb[i], kb[k],
 *     dup_overlap) for a slot k kept before it (the first such k in that order).  A suppressed slot: dup_of[i] = k, lost[i] = 1,
 *     next_boxes[i] = 0 0 0 0, lost_count[i] = 0.  dup_of = -1 for every other slot of a frame.
 *  4. lost_count = 0 for a kept slot and for one with src_frame < 0; every other slot that is not suppressed counts
 *     min(lost_count + 1, 1 << 30), and with max_lost > 0 a count >= max_lost empties it: next_boxes = 0 0 0 0, lost_count = 0.
 *  5. The frame's free slots are those not kept, in ascending index.  Its valid detections are walked in descending score (ties:
 *     lower index): det_state[d] = -2 if over(det, kb[i], match_overlap) for a kept slot i, else -3 if it overlaps (same test) a
 *     detection accepted before it, else -4 if no free slot is left, else the first free slot i: seeded[i] = d, next_boxes[i] = the
 *     detection's box, next_rot[i] = (1, 0), lost_count[i] = 0 (lost[i] stays as it is).  det_state = -1 for every other entry,
 *     seeded = -1 for every other slot of a frame.
 * One workgroup of 64 threads per frame (a mode of the fp32 frame-crop kernel with a launch of its own and dynamic LDS sized by b and k);
 * records staged in LDS, ranks by counting, no atomics: a replay is bit-reproducible.
 * 1 <= b <= 1024, 1 <= k <= 1024, j > 0; thresholds finite, and all but track_min_score >= 0; max_lost >= 0. */
int lh_tracks_manage(const float* preds_dev, const float* maxvals_dev, const int* src_frame_dev, const int* frame_index_dev, int b, int j,
                     int n_frames, const float* det_boxes_dev, const int* det_frame_dev, const float* det_score_dev, int k,
                     float track_min_score, float track_min_side, float dup_overlap, float match_overlap, float det_min_score, int max_lost,
                     float* next_boxes_dev, float* next_rot_dev, int* lost_dev, int* lost_count_dev, int* dup_of_dev, int* seeded_dev,
                     int* det_state_dev, void* stream);
/* Motion-aware tracking (opt-in; runtime.ManagedInferStep(frames=..., track=True, motion=..., smooth=..., smooth_gate=...)).  All
 * arithmetic is fp32 in the order written, with + - * /, fabsf, fminf / fmaxf and comparisons only.
 * lh_rois_predict: ROI velocity prediction and coasting, one launch behind lh_keypoints_to_boxes / lh_keypoints_to_rois and
 * lh_tracks_manage and in front of the filter.  It edits next_boxes_dev fp32 [b][4] in place -- a translation, so it serves upright
 * and oriented ROIs alike -- and keeps the state centre_dev fp32 [b][2], vel_dev fp32 [b][2] (frame px / s), seen_dev int32 [b],
 * coasted_dev int32 [b].  lost_dev, src_frame_dev int32 [b], seeded_dev int32 [b] (lh_tracks_manage's; may be NULL) and dt_dev fp32
 * [b] (seconds since the slot's previous frame) are read.  Slot i, (x0, y0, x1, y1) its incoming box, okdt = dt > 0 && isfinite(dt):
 *  1. reset -- src_frame < 0, or seeded[i] >= 0, or !(x1-x0 > 0 && y1-y0 > 0): seen = 0, vel = 0, coasted = 0; the box stays.
 *  2. lost != 0: if seen && okdt && coasted < coast: s = vel * dt per axis clamped to +-lim (step 3's), added to the box and to centre,
 *     ++coasted; otherwise seen = 0, vel = 0.
 *  3. found: c = ((x0+x1)*0.5, (y0+y1)*0.5).  If !seen || !okdt: centre = c, vel = 0, seen = 1, coasted = 0, no shift.  Otherwise
 *     vm = (c - centre) / dt, r = (6.2831855f * cutoff) * dt, a = r / (r + 1.f), vel = a * vm + (1.f - a) * vel (lh_one_euro's
 *     derivative low-pass); centre = c, coasted = 0; a vel that is not finite becomes 0 and nothing moves; else
 *     lim = max_shift * fmaxf(x1-x0, y1-y0), s = fminf(fmaxf((lead * vel) * dt, -lim), lim) per axis, added to x0, x1 / y0, y1.
 * One thread per slot, no atomics.  cutoff (Hz) > 0, lead >= 0, max_shift >= 0, all finite; coast >= 0; b > 0.
 * lh_one_euro_gated: lh_one_euro with a confidence gate per joint and, with by_size != 0, beta multiplying a speed in hand sizes per
 * second; in lh_one_euro's place, never beside it.  x_dev, xhat_dev, dxhat_dev, out_dev as lh_one_euro's; maxvals_dev fp32 [b][j];
 * next_boxes_dev fp32 [b][4] (read with by_size only; may be NULL without); state seen_j_dev int32 [b][j] (in the place of init) and
 * gap_dev fp32 [b][j], the seconds a joint has gone without an update.  An away slot (src_frame < 0, or lost_dev non-NULL and set)
 * passes x through and zeroes its seen_j and gap.  Otherwise per joint: gated out (!(maxval >= gate_min_score)): out = seen_j ? xhat :
 * x, the state stays, gap += dt when dt > 0 and finite.  Gated in: T = gap + dt; if !seen_j or T is not > 0 and finite: xhat = x,
 * dxhat = 0, out = x; else lh_one_euro's update with T for dt and fc = min_cutoff + beta * speed, speed = fabsf(dxhat'), or with
 * by_size fabsf(dxhat') / fmaxf(fmaxf(x1-x0, y1-y0), 1.f); then seen_j = 1, gap = 0.  With gate_min_score = -3.0e38f, by_size = 0 and
 * finite maxvals, out / xhat / dxhat are lh_one_euro's bit for bit over any sequence of frames (T = 0 + dt).  One workgroup of 64
 * threads per slot, one thread per coordinate (strided); a joint's seen_j and gap are written by one thread behind a barrier. */
int lh_rois_predict(float* next_boxes_dev, const int* lost_dev, const int* src_frame_dev, const int* seeded_dev, const float* dt_dev, int b,
                    float cutoff, float lead, float max_shift, int coast, float* centre_dev, float* vel_dev, int* seen_dev, int* coasted_dev,
                    void* stream);
int lh_one_euro_gated(const float* x_dev, const float* maxvals_dev, const float* next_boxes_dev, const int* src_frame_dev, const int* lost_dev,
                      const float* dt_dev, int b, int j, float min_cutoff, float beta, float d_cutoff, float gate_min_score, int by_size,
                      float* xhat_dev, float* dxhat_dev, int* seen_j_dev, float* gap_dev, float* out_dev, void* stream);
/* Skeleton overlay (opt-in; runtime.ManagedInferStep(frames=..., overlay=...)): the tracked hands drawn into the frames IN PLACE, on
 * the pixels around each hand only.  The frames are EITHER frames with frame_stride OR surface_table_dev, and layout says where their
 * texels are, all three as lh_frames_crop_surfaces_to_nhwc4's (chroma_siting and csc12 are checked and not used: the kernel converts
 * no colour and ignores chroma siting).  Per slot: preds_dev fp32 [b][j][2] (frame coordinates, pixel centres on the integers),
 * maxvals_dev fp32 [b][j], src_frame_dev int32 [b], lost_dev int32 [b] (may be NULL), mat_dev fp32 [b][6] the slot's crop matrix of a
 * crop_h x crop_w crop (may be NULL: no outline), boxes_dev fp32 [b][4] (may be NULL with by_size == 0).  parents_dev int32 [j] (-1 or
 * outside 0..j-1: no bone), group_dev int32 [j] (the palette row of joint i and of the bone that ends in i), palette_dev fp32
 * [n_groups + 2][3] in the frames' own plane space (R G B on 0..255; Y Cb Cr on the 8-bit scale, for p010 on the 10-bit scale); its
 * last two rows colour the outline of a live and of a lost slot.  All arithmetic is fp32 in the order written.
 *  s = by_size != 0 ? (bw > bh ? bw : bh) of the slot's box : 0, r_line = line_radius + by_size*s, r_joint = joint_radius + by_size*s.
 *  The primitives of a slot, in this order: with mat_dev and draw_roi the four edges c0c1, c1c2, c2c3, c3c0 of the crop's quad, c =
 *  (-.5, -.5), (w-.5, -.5), (w-.5, h-.5), (-.5, h-.5) through the matrix as the crop takes a pixel (fx = (m0*u + m1*v) + m2), radius
 *  r_line, row n_groups, or n_groups + 1 for a lost slot (lost != 0), which draws nothing else; the bones i = 0..j-1 with a parent,
 *  from joint parents[i] to joint i, when both maxvals are >= min_score, radius r_line, row group[i]; the joints i = 0..j-1 with
 *  maxval >= min_score as segments of length 0, radius r_joint, row group[i].  A primitive with a coordinate or radius that is not
 *  finite, or a row outside the palette, is skipped.  A slot with src_frame outside 0..n_frames-1, or on an unbound surface (table
 *  entry 0, tested before an address is formed), draws nothing.
 *  Coverage of the pixel (px, py) by the segment a -> b of radius r: d = (b - a), l2 = dx*dx + dy*dy, q = p - a, e = q; if l2 > 0:
 *  t = (qx*dx + qy*dy) * (1.f / l2) clamped to 0..1 by comparison, e = q - t*d; k = (r + 0.5f) - sqrtf(ex*ex + ey*ey) clamped to
 *  0..1 by comparison (a bone of length 0 is the disc of its end point).
 *  A pixel starts from its texel as a float; for every primitive of every slot of its frame, slot after slot in index order, with
 *  al = opacity * k > 0: c = c + al * (colour - c) per component; it ends as floorf(c + 0.5f) clamped to the texel range, and a
 *  pixel no primitive covers is NOT WRITTEN.  4:2:0 frames: luma is such a plane; the chroma pair of a 2 x 2 luma block takes
 *  al = (opacity * ((k00 + k01) + (k10 + k11))) * 0.25f and the palette's Cb / Cr.  p010 blends u16 >> 6 on the 10-bit scale
 *  (0..1023) and stores code << 6; a texel that is not written keeps its low six bits.
 * b * 8 workgroups of 256 threads, each walking its slot's draw bounds (the primitives' bounds grown by r + 1, clipped to the frame)
 * in a grid-stride loop: nothing runs over whole frames, nothing is read or written outside a frame.  A pixel is owned by the lowest
 * drawing slot of its frame whose bounds contain it, and the owner composites every slot whose bounds contain it: one writer per
 * texel, no atomics, a replay is bit-reproducible.  (A mode of the fp32 frame-crop kernel with a launch of its own and dynamic LDS
 * sized by b.)  LH_ERR_ARG: a NULL pointer beside those named; b outside 1..1024; j, n_groups, n_frames, crop_h or crop_w < 1;
 * a radius or by_size that is negative or not finite, min_score not finite, opacity outside 0..1; the frame source and layout as
 * lh_frames_crop_surfaces_to_nhwc4's; palette_dev equal to preds_dev or maxvals_dev. */
int lh_draw_hands(unsigned char* frames, long frame_stride, const long long* surface_table_dev, const lh_frames_layout* layout, int n_frames,
                  int hs, int ws, const float* preds_dev, const float* maxvals_dev, const int* src_frame_dev, const int* lost_dev,
                  const float* mat_dev, const float* boxes_dev, int b, int j, int crop_h, int crop_w, const int* parents_dev,
                  const int* group_dev, const float* palette_dev, int n_groups, float min_score, float line_radius, float joint_radius,
                  float by_size, float opacity, int draw_roi, void* stream);
/* Training on hand ROIs cropped from full frames (opt-in; runtime.TrainStep(frames=..., roi_aug=...)).
 * lh_roi_perturb: the caller's ROI (boxes_dev fp32 [b][4], rot_dev fp32 [b][2] or NULL = (1, 0), mirror_dev int32 [b] or NULL = 0) and
 * this step's draw aug_dev fp32 [b][6] = (c, s, k, tx, ty, flip) -> the ROI that lh_roi_affine reads (boxes_out, rot_out, mirror_out).
 * (c, s) = (cos, sin) of the drawn rotation, k the scale of the extents, (tx, ty) a shift of the centre along the ROI's own axes as a
 * fraction of its extents, flip != 0 toggles the mirror.  One thread per slot, no atomics, no sinf / cosf; fp32 in this order:
 *   bw = x1-x0, bh = y1-y0, cx = (x0+x1)*0.5, cy = (y0+y1)*0.5
 *   n = sqrtf(rx*rx + ry*ry), ux = rx/n, uy = ry/n
 *   dx = tx*bw, dy = ty*bh, cx' = cx + (dx*ux - dy*uy), cy' = cy + (dx*uy + dy*ux)
 *   hw = (bw*k)*0.5, hh = (bh*k)*0.5, box' = (cx'-hw, cy'-hh, cx'+hw, cy'+hh)
 *   rot' = (ux*c - uy*s, ux*s + uy*c)
 *   mirror' = (mirror != 0) != (flip != 0) ? 1 : 0
 * A slot whose aug row is exactly (1, 0, 1, 0, 0, 0) copies box, rot and mirror bit for bit (rot is not normalised): no augmentation
 * is the un-augmented crop.  A box, rot or aug row that is not finite, or n not > 0, copies box, rot and mirror as well (lh_roi_affine
 * turns such a ROI into an empty slot).  No output may be one of the inputs: LH_ERR_ARG. */
int lh_roi_perturb(const float* boxes_dev, const float* rot_dev, const int* mirror_dev, const float* aug_dev, int b, float* boxes_out,
                   float* rot_out, int* mirror_out, void* stream);
/* The position lh_affine_points_inv gives the points of a slot it cannot map: every target renderer treats it as off the map (a zero
 * plane, target weight 0). */
#define LH_POINT_OFF (-65536.f)
/* The twin of lh_affine_points: pts (frame coordinates, pstride floats per point) through the INVERSE of mat_dev fp32 [b][6]
 * (crop pixel index -> frame pixel index, lh_box_affine's / lh_roi_affine's) into out (crop coordinates, ostride floats per point).
 * One thread per point, fp32 in this order: det = m0*m4 - m1*m3, qx = x - m2, qy = y - m5, ox = (m4*qx - m1*qy) / det,
 * oy = (m0*qy - m3*qx) / det.  An empty slot (src_frame_dev[slot] < 0), or det not finite or == 0, writes (LH_POINT_OFF,
 * LH_POINT_OFF).  The matrix (1, 0, 0, 0, 1, 0) returns the points' own bits.  Columns past the first two are not read or written. */
int lh_affine_points_inv(const float* pts, int pstride, const float* mat_dev, const int* src_frame_dev, float* out, int ostride, int b,
                         int j, void* stream);
/* NHWC (run dtype) -> NCHW fp32 heatmaps (what model(images) returns, pose_resnet.py:246)
 * and the inverse for the incoming gradient. c_stride = channel stride of the NHWC side. */
int lh_nhwc_to_nchw_f32(const void* nhwc, float* nchw, int n, int h, int w, int c, int c_stride,
                        int dtype, void* stream);
int lh_nchw_f32_to_nhwc(const float* nchw, void* nhwc, int n, int h, int w, int c, int c_stride,
                        int dtype, void* stream);

/* ------------------------------------------------------------------ weight packs
 * Build the K-major device image [Cout_pad128][ntaps][Kpad] of one tap subset of a
 * weight tensor.  Logical weight element (o, i, r, s) is read from
 * w[o*so + i*si + r*sr + s*ss] (fp32, reference layout via strides), taps are listed as
 * (r, s) pairs; rows o >= n_out and columns i >= n_in are zero.  Returns packed bytes
 * through *bytes when out == NULL (size query). */
int lh_pack_weight(const float* w, void* out, size_t* bytes, int n_out, int n_in,
                   long so, long si, long sr, long ss, int ntaps, const int* taps_rs,
                   int dtype, void* stream);

/* The same for every pack of a model in one launch: `items` is a DEVICE array of descriptors. */
typedef struct {
    const float* w;
    void* out;
    int n_out, n_in, ntaps, pad_;
    long so, si, sr, ss;
    signed char r[64];
    signed char s[64];
} lh_pack_item;
/* chunk tables (device): chunk j rebuilds elements [chunk_start[j], +lh_pack_chunk_elems()) of pack chunk_item[j] */
int lh_pack_chunk_elems(void);
int lh_pack_weights_multi(const lh_pack_item* items_dev, const int* chunk_item_dev, const long* chunk_start_dev,
                          int n_chunks, int dtype, void* stream);

/* Regular weight tensors w[d0][d1][kH*kW] (Conv2d: d0 = C_out, d1 = C_in; ConvTranspose2d: d0 = C_in, d1 = C_out):
 * every pack of every such tensor in one launch, through 32 x 32 x taps LDS tiles (coalesced reads, 64-byte writes).
 * A pack is [rows pad128][ntaps][kpad] with rows = d1 (row_is_d1) or d0; taps[] index kH*kW positions (r*kW + s).
 * Padding of the pack images must be zero beforehand (it is never written).  chunk tables (device int32): chunk j
 * handles tile (t0[j], t1[j]) (units of 32) of tensor conv[j]. */
typedef struct {
    void* out;
    int row_is_d1, ntaps, kpad, pad_;
    int taps[16];
} lh_pack_out;
typedef struct {
    const float* w;
    int d0, d1, rs, npacks;
    lh_pack_out packs[5];
} lh_pack_conv;
int lh_pack_weights_tiled(const lh_pack_conv* convs_dev, const int* chunk_conv_dev, const int* chunk_t0_dev,
                          const int* chunk_t1_dev, int n_chunks, int max_rs, int dtype, void* stream);

/* ------------------------------------------------------------------ convolutions
 * nn.Conv2d(..., bias=False) + the head conv with bias: pose_resnet.py:23-26,66-72,152,
 * 169-175,181-182; pose_hrnet.py:22-25,65-71,145-149,200-204,218-222,230-234,282-286,
 * 323-329,344-348,363-365,378-381.  nn.ConvTranspose2d(k=4,s=2,p=1): pose_resnet.py:219-227.
 *
 * One descriptor covers forward, data-gradient and transposed forms: an output pixel
 * grid (ho, wo) per image, a list of taps (dh, dw) that select the input pixel
 * (a*sh + dh, b*sw + dw) and the weight-pack slice, and an affine placement of the
 * output pixel (a*osh + ooh, b*osw + oow) inside an [OH][OW] image (used by the four
 * sub-pixel phases of stride-2 transposed convolutions). */
typedef struct {
    int n, hi, wi;            /* input batch / image size in pixels                  */
    int in_pix_stride;        /* elements between adjacent input pixels              */
    int k_run;                /* valid contiguous elements per tap                   */
    int ho, wo;               /* output pixel grid of this launch                    */
    int sh, sw;               /* input sampling stride                               */
    int cout;                 /* valid output channels                               */
    int OH, OW;               /* full output image size                              */
    int osh, osw, ooh, oow;   /* output pixel = (a*osh + ooh, b*osw + oow)           */
    int out_pix_stride;       /* elements between adjacent output pixels             */
    int ntaps;
    int relu;                 /* apply max(.,0) before the store                     */
    signed char dh[64];
    signed char dw[64];
    /* Kernel configuration chosen by the caller (all zero = the library's static default).  cfg[0..4] = convolution
     * kernel: tile output channels, tile pixels, ring depth, K bytes per ring stage, reserved (0); ring depth 1 selects
     * the persistent pointwise kernel (1x1, dense output, K <= 512, 16-bit types): channels of the resident weight
     * panel, pixels a wave takes per step, 1, padded K of the panel
     * -- one of lh_igemm_candidates().  cfg[5..7] = weight-gradient kernel (lh_wgrad*): tile output channels, tile
     * input channels, pixel splits -- one of lh_wgrad_candidates().  Results do not depend on cfg[0..4]; the
     * weight gradient's fp32 summation order depends on the split count (deterministic for a given cfg). */
    int cfg[8];
} lh_igemm_desc;

/* out[pixel][co] = relu?( (sum_taps sum_k in[pix(tap)][k] * wpack[co][tap][k] + bias[co]) * scale[co] + shift[co]
 *                          + addend[pixel][co] )      (bias / scale+shift / addend optional; relu from the descriptor).
 * scale/shift fold an eval-mode BatchNorm (and with addend + relu a whole residual-unit tail) into the epilogue.
 * addend_mask (optional, dense outputs only): the relu_mask bits lh_fuse_fwd stored for an activation; element e of a
 * 16-byte chunk of the addend is added only where its bit is set.  Lets a data-gradient launch add the identity-shortcut
 * gradient of a residual tail, dout * (out > 0), straight from dout (loss.backward() through `out += residual; relu`,
 * pose_resnet.py:96-97) instead of reading a copy lh_fuse_bwd would have to write first.
 * stats (optional): fp32 [gridM][2][cout] per-block column sums / sums of squares of the stored values,
 * consumed by lh_bn_finalize.  addend may alias out. */
int lh_igemm(const lh_igemm_desc* d, const void* in, const void* wpack, void* out,
             const void* addend, const void* addend_mask, const float* bias, const float* scale, const float* shift,
             float* stats, int dtype, void* stream);
/* A data-gradient launch whose OUTPUT is the gradient of an activation a = relu(BN(x)) (x = the forward convolution's raw
 * output, BN in training mode: pose_resnet.py:60-66 and what loss.backward() does with them) can do the first half of that
 * BatchNorm's backward pass on the tile it holds: it stores g = dout * (x * scale + shift > 0) -- the ReLU-gated gradient
 * -- instead of dout, and writes the per-block partial sums { sum g, sum g * (x - mean) * invstd } per channel into `partial`
 * (fp32 [rows][2][cout], rows = lh_igemm_stats_rows: the layout of the forward statistics).  lh_fuse_bwd then takes them
 * (lh_fuse_bwd_desc.pre_partial / pre_rows) and skips its own reduce pass over dout and x: one read of dout, one launch
 * less per BatchNorm.  x has the layout of this launch's output (same pixel stride).
 * mask (optional; dense outputs): the activation is a residual tail a = relu(BN(x) + r) (`out += residual; relu`,
 * pose_resnet.py:96-97) -- its sign does not follow from x alone, it is read from the relu_mask bits lh_fuse_fwd stored for the tail
 * (scale / shift are then unused and may be NULL).  x2 (optional, with mask; pointwise kernel only): r is a projection shortcut
 * BN2(x2) (`residual = self.downsample(x)`, pose_resnet.py:93-94) -- partial2 takes { sum g, sum g * (x2 - mean2) * invstd2 }.
 * `partial` / `partial2` have lh_igemm_gated_rows(d, dtype, nterms = 1 | 2) rows.
 * Tiled LDS-DMA configurations (lh_igemm_config: ring depth 2..9 and the dense-wave forms) and the persistent pointwise kernel
 * (ring depth 1); LH_ERR_UNSUPPORTED otherwise. */
typedef struct {
    const void* x;
    const float* mean;
    const float* invstd;
    const float* scale;
    const float* shift;
    float* partial;
    const void* mask;
    const void* x2;
    const float* mean2;
    const float* invstd2;
    float* partial2;
} lh_bn_bwd_gate;
int lh_igemm_gated_rows(const lh_igemm_desc* d, int dtype, int nterms);
int lh_igemm_gated(const lh_igemm_desc* d, const void* in, const void* wpack, void* out, const void* addend, const void* addend_mask,
                   const lh_bn_bwd_gate* gate, int dtype, void* stream);
/* Phase batching: 2..4 lh_igemm launches that share input, output tensor, sizes and epilogue and differ only in weight
 * pack, tap list and output placement (ooh, oow) -- the sub-pixel phases of a 4x4/s2 transposed convolution
 * (pose_resnet.py:194-232) or of a stride-2 convolution's data gradient -- as ONE grid.  Phases may have zero taps
 * (they store addend / bias only).  stats: nphase * lh_igemm_phases_rows(..) rows, phase p's rows at p * rows.
 * Requires the LDS-DMA kernel (16-byte aligned rows, regular tap grids); returns LH_ERR_* otherwise. */
int lh_igemm_phases_rows(const lh_igemm_desc* const* descs, int nphase, int dtype);
int lh_igemm_phases(const lh_igemm_desc* const* descs, int nphase, const void* in, const void* const* wpacks,
                    void* out, const void* addend, const void* addend_mask, const float* bias, const float* scale,
                    const float* shift, float* stats, int dtype, void* stream);
/* Inference head (pose_resnet.py:245-246 with eval-mode BatchNorm: x = relu(bn(deconv(x))); x = final_layer(x)): the
 * sub-pixel phases of the LAST transposed convolution with the folded BatchNorm affine and ReLU, and the 1x1 final layer
 * applied to every output tile while it is still in LDS -- the C-channel activation never reaches HBM, only the fp32
 * NCHW heat-map [n][n_out][OH][OW] is written.  Needs the 256 x 256 tile (descs[*]->cfg), cout <= 256, a 16-bit type.
 * head.w: K-major rows [>= 32][w_row_bytes] of the 1x1 weight in the run precision (rows >= n_out zero: the pack
 * lh_pack_weight makes for that convolution), head.bias: fp32 [n_out] or NULL. */
typedef struct {
    const void* w;
    size_t w_row_bytes;
    const float* bias;
    float* out;
    int n_out;
} lh_head;
int lh_igemm_phases_head(const lh_igemm_desc* const* descs, int nphase, const void* in, const void* const* wpacks,
                         const float* scale, const float* shift, const lh_head* head, int dtype, void* stream);
/* tile (output channels x pixels) the dispatcher picks for this descriptor: names the kernel
 * instantiation a launch uses -- igemm_ring_kernel<T, bm, bp, .., depth, kbytes> when *ring != 0 (LDS-DMA ring
 * path, 16-byte aligned pixel rows; *ring = kbytes*10 + depth) else igemm_kernel<T, bm, bp, ..>. */
int lh_igemm_tile(const lh_igemm_desc* d, int dtype, int* bm, int* bp, int* ring);
/* The configuration a launch of this descriptor runs with (cfg5 = tile channels, tile pixels, ring depth, K bytes per
 * stage, 0; depth 0 = the register-staged kernel), and the configurations compiled in that fit it
 * (5 ints each, returns the count; 0 when the form only runs on the register-staged kernel): the plan times them on
 * the real buffers and writes the winner into lh_igemm_desc.cfg (lighthand_amd/engine.py, Plan._tune). */
int lh_igemm_config(const lh_igemm_desc* d, int dtype, int* cfg5);
int lh_igemm_candidates(const lh_igemm_desc* d, int dtype, int* cfgs, int max);
/* Weight gradient of a convolution whose kernel rows are separate "row taps" (the C_in = 3 stem on NHWC4: a kernel row =
 * one contiguous run of k pixels x 4 channels, pose_resnet.py:152) with ALL rows in one pass: d describes ONE tap (the
 * first kernel row) and has k_run = rows * run; gradient input index i = row * run + k is read at input row ih + row,
 * element k of the run.  dy is read once per input tile instead of once per kernel row.  Slab / fold as for lh_wgrad with
 * the same descriptor (ntaps = 1, n_in = d->k_run).  LDS-DMA kernel only (16-bit types, 16-byte aligned runs). */
int lh_wgrad_rowfold(const lh_igemm_desc* d, int rows, const void* x, const void* dy, int dy_pix_stride,
                     int n_out, float* slab, int dtype, void* stream);
int lh_wgrad_tile(const lh_igemm_desc* d, int n_out, int n_in, int dtype, int* bo, int* bi, int* nsplit, int* ring);
/* Launch plans of the LDS-DMA weight-gradient kernel that fit this descriptor: 5 ints each = { tile output channels,
 * tile input channels, cfg[7] encoding (splits | stage rows << 16 | ring depth << 24), workgroups, slab MiB }.  Writing
 * the first three into lh_igemm_desc.cfg[5..7] selects the plan for lh_wgrad / lh_wgrad_slab_bytes / lh_wgrad_reduce
 * (0 when only the register-staged kernel applies: fp32, unaligned pixel rows). */
int lh_wgrad_candidates(const lh_igemm_desc* d, int n_out, int n_in, int dtype, int* out, int max);
/* n independent lh_igemm launches (one entry = the arguments of lh_igemm) as ONE grid: every descriptor's cfg must name the
 * same TILED configuration (ring depth >= 2, a 4-wave tile, 16-bit types); the same layer position of HRNet's parallel
 * branches (pose_hrnet.py:139-185).  Statistics slabs, addends, epilogue vectors are per problem. */
typedef struct {
    const lh_igemm_desc* d; const void* in; const void* wpack; void* out; const void* addend; const void* addend_mask;
    const float* bias; const float* scale; const float* shift; float* stats;
} lh_igemm_call;
int lh_igemm_multi(const lh_igemm_call* calls, int n, int dtype, void* stream);
/* rows of the stats slab lh_igemm writes for this descriptor (= number of pixel tiles) */
int lh_igemm_stats_rows(const lh_igemm_desc* d, int dtype);

/* Weight gradient (loss.backward(), src/utils/method.py:182):
 *   dW[tap][o][i] = sum_pixels dy[pixel][o] * x[pix(tap)][i]
 * with the same tap/gather description (x is the gathered operand, dy is dense
 * [n*ho*wo][dy_pix_stride]).  Partial sums go to `slab` (fp32, lh_wgrad_slab_bytes), then
 * lh_wgrad_reduce folds the split-K slabs into the reference-layout gradient
 * grad[o*so + i*si + r*sr + s*ss] (accumulate != 0 adds to what is there). */
size_t lh_wgrad_slab_bytes(const lh_igemm_desc* d, int n_out, int n_in, int dtype);
int lh_wgrad(const lh_igemm_desc* d, const void* x, const void* dy, int dy_pix_stride,
             int n_out, int n_in, float* slab, int dtype, void* stream);
int lh_wgrad_reduce(const lh_igemm_desc* d, const float* slab, float* grad, int n_out, int n_in,
                    long so, long si, long sr, long ss, const int* taps_rs, int accumulate,
                    int dtype, void* stream);
/* Both steps as one call: lh_wgrad (rows <= 1) or lh_wgrad_rowfold (rows > 1) into `workspace`
 * (lh_wgrad_workspace_bytes, device; launches that run one after another on a stream may share it), then lh_wgrad_reduce
 * into `grad`. */
size_t lh_wgrad_workspace_bytes(const lh_igemm_desc* d, int n_out, int n_in, int dtype);
/* n independent lh_wgrad_fused calls (one entry = its arguments; every problem needs its OWN workspace) as one weight-gradient
 * launch + one fold launch where tile / stage / ring depth agree (cfg[5..7]; 4-wave tiles), one by one otherwise. */
typedef struct {
    const lh_igemm_desc* d; int rows; const void* x; const void* dy; int dy_pix_stride, n_out, n_in; void* workspace; float* grad;
    long so, si, sr, ss; const int* taps_rs; int accumulate;
} lh_wgrad_call;
int lh_wgrad_fused_multi(const lh_wgrad_call* calls, int n, int dtype, void* stream);
int lh_wgrad_fused(const lh_igemm_desc* d, int rows, const void* x, const void* dy, int dy_pix_stride, int n_out, int n_in,
                   void* workspace, float* grad, long so, long si, long sr, long ss, const int* taps_rs, int accumulate,
                   int dtype, void* stream);
/* Table launches -- the deferred weight gradients of a whole stage (loss.backward(), src/utils/method.py:182, through the blocks of
 * one layerN of pose_resnet.py:61-99,177-192 or the branches of one HighResolutionModule, pose_hrnet.py:247-265) as ONE grid of the
 * LDS-DMA weight-gradient kernel plus at most ONE fold grid, whatever their number and shapes.  lh_wgrad_table_build (host only, once
 * per plan: every pointer of a plan is static) turns n lh_wgrad_call entries (16-bit types, rows <= 1; their `workspace` fields are
 * ignored) into a table blob the caller uploads to device memory: argument blocks + work-item lists.  cfg4 = { tile output channels,
 * tile input channels, pixel rows per ring stage, ring depth } (one of the compiled-in configurations, see lh_wgrad_candidates);
 * EVERY PROBLEM GETS ITS OWN PIXEL-SPLIT COUNT: work items of about `target_stages` ring stages each (0 = automatic: split-free when
 * the tiles alone fill the machine twice, else about four rounds of its workgroup slots), ordered longest first.  A problem with one
 * split, one tap and a gradient that is dense in [o][i] is written by the kernel itself (no slab, no fold entry).  The sums are a
 * deterministic function of (calls, cfg4, target_stages).  Call with host_blob = NULL to size the blob and the shared fp32 slab
 * workspace (info->table_bytes, info->workspace_bytes; runs without a device), then with both buffers.  lh_wgrad_table_run replays it:
 * `table` = the device copy of the blob. */
typedef struct {
    int bo, bi, kps, depth;              /* kernel configuration */
    int n_problems, n_fold;              /* problems in the table, problems that need the fold launch */
    int n_items, n_fold_items;           /* workgroups of the weight-gradient launch / of the fold launch (0: no fold launch) */
    int fold_lds, target_stages, nsplit_max;
    int run_parts;                       /* lh_wgrad_table_run: 0 = both launches, 1 = the weight-gradient grid only, 2 = the fold grid only (timing) */
    size_t off_items, off_fold_args, off_fold_items, table_bytes, workspace_bytes;
} lh_wgrad_table_info;
int lh_wgrad_table_build(const lh_wgrad_call* calls, int n, int dtype, const int* cfg4, int target_stages, void* workspace,
                         void* host_blob, size_t host_bytes, lh_wgrad_table_info* info);
int lh_wgrad_table_run(const void* table, const lh_wgrad_table_info* info, int dtype, void* stream);

/* ------------------------------------------------------------------ BatchNorm / fused elementwise
 * nn.BatchNorm2d(C, momentum=0.1): pose_resnet.py:19,35,... ; nn.ReLU / residual add:
 * pose_resnet.py:55-56,96-97; nn.Upsample(nearest): pose_hrnet.py:207. */

/* Column sums / sums of squares of a dense [m][c] activation -> stats slab [rows][2][c]. */
int lh_bn_stats(const void* y, int m, int c, float* stats, int* rows_out, int dtype, void* stream);
int lh_bn_stats_rows(int m, int c);
/* Bytes a stats slab of `rows` rows and `c` channels must have (slab + fp64 fold scratch). */
size_t lh_bn_stats_slab_bytes(int rows, int c);
/* Fold a stats slab: batch mean / biased var -> scale = gamma*rsqrt(var+eps),
 * shift = beta - mean*scale, saved mean / invstd; running stats updated with momentum and
 * the unbiased variance, num_batches_tracked (int64) += 1 (all device pointers). */
int lh_bn_finalize(const float* stats, int rows, int count, int c, const float* gamma,
                   const float* beta, float* running_mean, float* running_var,
                   long long* num_batches_tracked, float momentum, float eps, float* scale,
                   float* shift, float* save_mean, float* save_invstd, void* stream);
/* n independent BatchNorm layers (one entry = the arguments of lh_bn_finalize) as one launch; see lh_fuse_fwd_multi. */
typedef struct {
    const float* stats; int rows, count, c; const float* gamma; const float* beta; float* running_mean; float* running_var;
    long long* num_batches_tracked; float momentum, eps; float* scale; float* shift; float* save_mean; float* save_invstd;
} lh_bn_finalize_call;
int lh_bn_finalize_multi(const lh_bn_finalize_call* calls, int n, void* stream);
/* Eval mode: scale/shift from running statistics. */
int lh_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int c, float* scale, float* shift,
                      void* stream);

/* out = relu?( sum_t term_t ),  term_t = up_t( x_t * scale_t + shift_t )   (scale_t NULL = identity).
 * Up to 4 terms; up_t is nearest-neighbour upsampling by 2^log2up of a [n][h>>l][w>>l][c] map. */
typedef struct {
    const void* x[4];
    const float* scale[4];
    const float* shift[4];
    int log2up[4];
    int nterms;
    int relu;
    void* relu_mask;            /* optional output: one byte per 16-byte chunk of `out`, bit e = (element e > 0); lets the
                                 * backward pass read n*h*w*c/8 mask bytes instead of the whole stored activation */
    const lh_bn_finalize_call* fin[4];
                                /* optional, per term: the BatchNorm finalize of that term (batch statistics -> scale / shift /
                                 * saved mean / invstd / running statistics: what lh_bn_finalize does) has NOT run yet and is part
                                 * of this call: the call launches the finalize first (all pending finalizes of a call, or of every
                                 * call of lh_fuse_fwd_multi, as ONE launch), then the elementwise kernel.  (Folding the statistics
                                 * inside the elementwise launch was measured slower and removed in round 6.)
                                 * fin[t]->scale / ->shift must equal scale[t] / shift[t].
                                 * ZERO-INITIALISE the descriptor (memset / = {0}): a caller compiled against the round-3 layout, or
                                 * one that fills the fields one by one, would otherwise pass garbage pointers here. */
    const void* l2_touch;       /* optional (round 5): l2_touch_bytes of device memory the NEXT launch on the stream reads first -- the
                                 * weight pack of the convolution that consumes `out`.  The streaming kernels read one word of every
                                 * 128-byte line of it in each XCD right before they end, so the convolution finds it in L2
                                 * (speed only; ignored by the kernels that have no such tail).  NULL / 0 = off. */
    size_t l2_touch_bytes;
} lh_fuse_desc;
int lh_fuse_fwd(const lh_fuse_desc* d, void* out, int n, int h, int w, int c, int dtype, void* stream);
/* Multi-problem forms (pose_hrnet.py:139-185, 247-265: the same layer position of the 2-4 parallel branches of a
 * HighResolutionModule): n INDEPENDENT calls -- one entry = the arguments of the single call -- run as one launch per
 * kernel instead of n (the argument blocks travel in the kernel-argument segment, four problems per launch).  Calls
 * that do not plan the same kernels (e.g. an upsampled term beside plain ones) run one by one: always legal, same results. */
typedef struct { const lh_fuse_desc* d; void* out; int n, h, w, c; } lh_fuse_fwd_call;
int lh_fuse_fwd_multi(const lh_fuse_fwd_call* calls, int n, int dtype, void* stream);
/* The planned route of a lh_fuse_fwd call with the same arguments, without launching anything (host arithmetic, no device
 * needed): *kind = the kernel (LH_FF_*), *grid = its workgroups.  For tests and tools that must know which kernel a shape takes. */
enum { LH_FF_GEN = 0,           /* any terms: up to four, upsampled ones, any chunk count */
       LH_FF_FLAT1 = 1,         /* one term, no upsampling, a power-of-two number <= 256 of 16-byte chunks per pixel */
       LH_FF_FLAT2 = 2 };       /* two such terms */
int lh_fuse_fwd_plan(const lh_fuse_desc* d, void* out, int n, int h, int w, int c, int dtype, int* kind, int* grid);

/* Backward of lh_fuse_fwd, two launches per BN term:
 *  reduce: sums[t] = { sum g_t, sum g_t * xhat_t } with g = dout * (out > 0), g_t = g summed over
 *          each upsampling cell;  apply: dx_t = scale_t * (g_t - mean(g_t) - xhat_t * mean(g_t xhat_t));
 *          identity terms get dx_t = g_t.  dgamma = sum g xhat, dbeta = sum g are written to
 *          dgamma/dbeta (fp32 [c]).  accumulate[t] != 0 adds into dx[t]. */
typedef struct {
    const void* dout;
    const void* out;            /* forward result (ReLU mask); NULL when relu == 0 */
    const void* x[4];           /* raw BN inputs (NULL for identity terms)          */
    const float* scale[4];
    const float* shift[4];      /* forward shift vectors (lets a single-BN-term ReLU mask be recomputed from x) */
    const float* save_mean[4];
    const float* save_invstd[4];
    void* dx[4];
    float* dgamma[4];
    float* dbeta[4];
    int log2up[4];
    int accumulate[4];
    int nterms;
    int relu;
    const void* relu_mask;      /* mask bits written by lh_fuse_fwd; when set, `out` is not read and may be NULL */
    int strips_cap;             /* 0 = default (512): upper bound on the strips of the streaming reduce pass = rows of the
                                 * partial-sum slab; 256 is the measured choice for nodes that share lh_fuse_bwd_multi launches */
    const float* pre_partial;   /* a ReLU node with ONE BN term -- alone, or beside one identity term (a residual tail) -- or with TWO BN
                                 * terms (a tail with a projection shortcut; pre_partial2 then holds term 1's sums) whose dout was written
                                 * by lh_igemm_gated: dout is already the gated gradient and these are its partial sums
                                 * [pre_rows][2][c] -- no reduce pass, no mask */
    int pre_rows;
    const void* l2_touch;       /* optional (round 5), as lh_fuse_desc.l2_touch: the last apply pass of the call warms these bytes in L2 */
    size_t l2_touch_bytes;
    const float* pre_partial2;  /* with pre_partial and two BN terms: the partial sums of term 1 (pre_partial: term 0), same rows */
} lh_fuse_bwd_desc;
size_t lh_fuse_bwd_workspace_bytes(int n, int h, int w, int c);
int lh_fuse_bwd(const lh_fuse_bwd_desc* d, int n, int h, int w, int c, void* workspace,
                int dtype, void* stream);
/* n independent nodes, each with its OWN workspace: their reduce / coefficient-fold / apply kernels as three launches. */
typedef struct { const lh_fuse_bwd_desc* d; int n, h, w, c; void* workspace; } lh_fuse_bwd_call;
int lh_fuse_bwd_multi(const lh_fuse_bwd_call* calls, int n, int dtype, void* stream);
/* The launch records a lh_fuse_bwd call with the same arguments consists of, in recorded order, without launching anything (host
 * arithmetic, no device needed; the pointers of the descriptor and the workspace are only tested for NULL).  Returns the number of
 * records (< 0: LH_ERR_*) and fills the first `cap` of them: kinds[i] = LH_FB_*, grids[i] = workgroups (a reduce record: its strips =
 * the rows of the term's partial-sum slab; an LH_FB_APPLY2 record is one kind and one grid for both terms), fold_rows[i] = the slab
 * rows the record's term folds inside its apply pass (0: a separate LH_FB_COEF record folds them; always 0 for LH_FB_COEF and
 * LH_FB_APPLY2 records -- the reduce records before an LH_FB_APPLY2 tell).  kinds / grids / fold_rows may be NULL. */
enum { LH_FB_REDUCE_GEN = 0,    /* partial sums of g, g * xhat: any chunk count, upsampled terms */
       LH_FB_REDUCE_FLAT = 1,   /* the same for l = 0 and a power-of-two number <= 256 of chunks per pixel */
       LH_FB_REDUCE_FLAT_X = 2, /* ... with the ReLU gate recomputed from x * scale + shift */
       LH_FB_COEF = 3,          /* coefficient fold of a slab: grid c / 16, or c / 4 from 256 rows on */
       LH_FB_APPLY_GEN = 4,
       LH_FB_APPLY_FLAT = 5,
       LH_FB_APPLY_FLAT_X = 6,
       LH_FB_APPLY2 = 7 };      /* both gradients of a two-term node without upsampling in one pass */
int lh_fuse_bwd_plan(const lh_fuse_bwd_desc* d, int n, int h, int w, int c, void* workspace, int dtype, int* kinds, int* grids,
                     int* fold_rows, int cap);

/* The inference stem of SimpleBaseline-ResNet as ONE launch: maxpool(relu(bn1(conv1(x)))) -- conv1 = nn.Conv2d(3, 64, 7, 2, 3),
 * bn1 in eval mode (running statistics folded into scale / shift), nn.MaxPool2d(3, 2, 1): src/modeling/simplebaseline/
 * pose_resnet.py:151-156 and the first four lines of PoseResNet.forward.  img: the zero-padded NHWC4 image the engine's input
 * transforms write ([n][hp][wp][4], image pixel (y, x) at (y + 3, x + 3)); wpack: the stem's weight pack (64 channels, one tap
 * per kernel ROW, K run = 8 pixels x 4 channels); out = [n][ph][pw][64] with ph = (conv_h - 1) / 2 + 1.  relu must be 1 (the
 * pool's padding is realised as zeros).  16-bit types.  Bit-identical to lh_igemm + lh_maxpool3x3s2_fwd on the same operands.
 * lh_stem_pool_grid: the workgroups the launch takes (persistent over tiles of 8 x 8 pooled pixels; host arithmetic only). */
int lh_stem_pool_grid(int n, int conv_h, int conv_w);
int lh_stem_pool(const void* img, int n, int hp, int wp, const void* wpack, const float* bias, const float* scale,
                 const float* shift, void* out, int conv_h, int conv_w, int relu, int dtype, void* stream);

/* The inference BOTTLENECK of the first ResNet stage as ONE launch (round 5):
 *   out = relu( bn3(conv3( relu(bn2(conv2( relu(bn1(conv1(x))) ))) )) + residual )
 * conv1 = 1x1 (cin -> 64), conv2 = 3x3 / stride 1 / pad 1 (64 -> 64), conv3 = 1x1 (64 -> 256), the BatchNorms in eval mode folded
 * into per-channel scale / shift (lh_bn_eval_affine): Bottleneck.forward, src/modeling/simplebaseline/pose_resnet.py:61-99, for the
 * blocks with stride 1 (pytorch and caffe style alike).  x = [n][h][w][cin], residual and out = [n][h][w][256] (residual = x for an
 * identity shortcut, the projection's output otherwise; out may alias neither).  w1 / w2 / w3: the weight packs lh_pack_weight makes
 * for those three convolutions (K-major rows, taps in (r, s) order).  16-bit types.  Only x and the residual are read and out is
 * written -- the two 64-channel intermediates stay in LDS.  Bit-identical to the three lh_igemm launches with the same folds.
 * lh_bottleneck_infer_grid: the workgroups the launch takes (persistent over 16 x 16 tiles; host arithmetic only, 0 for an empty problem). */
typedef struct { int n, h, w, cin, mid, cout; } lh_bottleneck_desc;
int lh_bottleneck_infer_grid(const lh_bottleneck_desc* d);
int lh_bottleneck_infer(const lh_bottleneck_desc* d, const void* x, const void* w1, const void* w2, const void* w3,
                        const float* s1, const float* b1, const float* s2, const float* b2, const float* s3, const float* b3,
                        const void* residual, void* out, int dtype, void* stream);

/* The TRAINING stem: conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False) alone (pose_resnet.py:151-152; bn1 runs on batch statistics),
 * same operands as lh_stem_pool (padded NHWC4 image, the stem's weight pack), on the same direct kernel form: out =
 * [n][conv_h][conv_w][64] raw convolution output (bit-identical to lh_igemm on that pack), stats = fp32
 * [lh_stem_conv_rows(n, conv_h, conv_w)][2][64] per-workgroup sums / sums of squares of the stored values for lh_bn_finalize.
 * lh_stem_conv_rows is the launch's grid as well (persistent over tiles of 16 x 16 outputs), as lh_stem_pool_grid and
 * lh_bottleneck_infer_grid are for theirs.  16-bit types. */
int lh_stem_conv_rows(int n, int conv_h, int conv_w);
int lh_stem_conv(const void* img, int n, int hp, int wp, const void* wpack, void* out, float* stats, int conv_h, int conv_w,
                 int dtype, void* stream);

/* nn.MaxPool2d(3, 2, 1): pose_resnet.py:156.  idx (uint8 [n][ho][wo][c]) keeps the window
 * position (first maximum in scan order, NaN propagates) for the backward pass; NULL when no backward pass follows. */
int lh_maxpool3x3s2_fwd(const void* x, void* out, unsigned char* idx, int n, int h, int w, int c,
                        int dtype, void* stream);
int lh_maxpool3x3s2_bwd(const void* dout, const unsigned char* idx, void* dx, int n, int h, int w,
                        int c, int dtype, void* stream);
/* lh_maxpool3x3s2_bwd whose output dx is the gradient of a = relu(BN(gate->x)) (the training stem: the pool follows bn1 + relu):
 * stores the ReLU-gated gradient and one row of BatchNorm-backward partial sums per workgroup (gate->partial: fp32
 * [lh_maxpool3x3s2_bwd_gated_rows][2][c]), for lh_fuse_bwd's pre_partial -- see lh_igemm_gated.  16-bit types. */
int lh_maxpool3x3s2_bwd_gated_rows(int n, int h, int w, int c, int dtype);
int lh_maxpool3x3s2_bwd_gated(const void* dout, const unsigned char* idx, void* dx, const lh_bn_bwd_gate* gate, int n, int h, int w,
                              int c, int dtype, void* stream);
/* maxpool(relu(bn(x))) of the training stem (pose_resnet.py:153-156: bn1, relu, maxpool) as ONE pass: x is the RAW BatchNorm
 * input, scale / shift the training-mode affine lh_bn_finalize derived from the batch statistics; every tap is
 * relu(x * scale + shift) rounded to the run precision -- the value lh_fuse_fwd would have stored -- so out and idx are
 * bit-identical to lh_fuse_fwd followed by lh_maxpool3x3s2_fwd, and the activation between them (the largest of the
 * network) is never written: the backward pass does not need it (lh_maxpool3x3s2_bwd works from idx, lh_fuse_bwd
 * recomputes the ReLU mask from x). */
int lh_bn_relu_maxpool3x3s2_fwd(const void* x, const float* scale, const float* shift, void* out, unsigned char* idx, int n,
                                int h, int w, int c, int dtype, void* stream);

/* ------------------------------------------------------------------ heatmap target / loss / decode */
/* CustomDataset.generate_target: src/tools/dataset.py:165-212.  joints fp32 [b][j][jstride]
 * (x, y in input pixels) -> fp32 [b][j][size][size].  `patch` is the (2*radius+1)^2 fp32
 * Gaussian the host evaluates exactly as the reference does (numpy float32 exp), so that the
 * placed values are bit-identical to the reference's on the same host. */
int lh_gaussian_target(const float* joints, int jstride, const float* patch, int radius,
                       float* target, int b, int j, int size, void* stream);
/* GenerateHeatmap.__call__: src/utils/dataset_loader.py:22-53 (the alternate renderer the reference's dataset classes
 * keep beside generate_target).  points fp32 [b][j][pstride] ALREADY in heat-map coordinates -> fp32 [b][j][res][res];
 * `patch` = the (6*sigma+3)^2 Gaussian the host evaluates in float64 like the reference and rounds to fp32 (what the
 * reference's float32 map stores); sigma = res / 64 must be an integer (the reference uses res = 64). */
int lh_gaussian_target_alt(const float* points, int pstride, const float* patch, int sigma,
                           float* target, int b, int j, int res, void* stream);
/* JointsMSELoss(use_target_weight=False): src/utils/loss.py:306-325.  loss (fp32 scalar on
 * device) = 0.5*mean((p-g)^2); grad (optional) = (p-g) * grad_scale/(numel). workspace >=
 * lh_mse_workspace_bytes(numel). */
size_t lh_mse_workspace_bytes(long numel);
int lh_mse_heatmap(const float* pred, const float* target, long numel, float* loss, float* grad,
                   const float* grad_scale, void* workspace, void* stream);
/* Opt-in extensions without a reference oracle (the reference computes target_weight, src/tools/dataset.py:171-186, and
 * never applies it; it has no hard-keypoint mining): the formulas are those of the SimpleBaseline / HRNet code line.
 *
 * lh_gaussian_target with upstream's target_weight: vis = optional fp32 visibility per joint, read at vis[i * vstride] for
 * joint i of b*j (NULL = 1); weight fp32 [b][j] = (vis > 0.5 ? vis : 0) * in_frame, in_frame = some part of the patch lies
 * inside the map (the negation of lh_gaussian_target's skip test).  target = lh_gaussian_target's, bit for bit, where
 * weight > 0 and a zero map otherwise (upstream's `if v > 0.5:`); with vis == NULL it is lh_gaussian_target's everywhere. */
int lh_gaussian_target_w(const float* joints, int jstride, const float* vis, int vstride, const float* patch, int radius,
                         float* target, float* weight, int b, int j, int size, void* stream);
/* DARK's unbiased target encoding (Zhang et al. 2020, upstream generate_target; an opt-in extension without a reference
 * oracle): the window, the skip test and the weight rule of lh_gaussian_target / lh_gaussian_target_w -- window of
 * (2 * radius + 1)^2 cells centred on mx = (int)(jx * 0.25f + 0.5f), weight = (vis > 0.5 ? vis : 0) * in_frame, a zero map where
 * the weight is 0, vis == NULL = 1 -- but the value inside the window is the Gaussian around the joint's real-valued position,
 * expf(-((x - jx * 0.25f)^2 + (y - jy * 0.25f)^2) / (2 * sigma^2)), evaluated per pixel in fp32 (no patch table).
 * weight == NULL: no weight output and no visibility test (vis is not read).  A joint on a cell centre jx = 4k, k >= 0, gets
 * lh_gaussian_target's map up to the rounding of expf (for k < 0 the truncation toward zero centres the window on k + 1). */
int lh_gaussian_target_sub(const float* joints, int jstride, const float* vis, int vstride, int radius, float sigma,
                           float* target, float* weight, int b, int j, int size, void* stream);
/* JointsMSELoss(use_target_weight=True) (topk == 0) and JointsOHKMMSELoss (1 <= topk <= j).  pred / target / grad fp32
 * [b][j][hw], weight fp32 [b][j] or NULL (ones), joint_loss optional fp32 [b][j], grad optional, grad_scale an optional
 * device scalar read on the device like lh_mse_heatmap's.  Per plane, fp64 in a fixed order (no atomics: every call gives the
 * same bits): S = w^2 * sum (float)(d * d), d = p - g in fp32; joint_loss = 0.5 * S / hw.
 * topk == 0: loss = 0.5 * sum S / (b*j*hw), grad = d * (w * w * gs), gs = (grad_scale ? *grad_scale : 1) / (float)(b*j*hw):
 *   one pass over pred / target plus one small launch; with weight == NULL grad is lh_mse_heatmap's bit for bit.
 * topk >= 1: per sample the topk largest joint_loss values are selected (fp32 values, the lower joint index among equals,
 *   a NaN first); loss = (1/b) sum_b (1/topk) sum_selected joint_loss; grad = d * (w * w * gs_k) on the selected planes,
 *   gs_k = scale / (float)(b*topk*hw), and exactly 0.f on the others.  Three launches: plane sums, select + loss, gradient.
 * Buffers 16-byte aligned, hw % 4 == 0 (LH_ERR_ARG otherwise); workspace >= lh_joints_mse_workspace_bytes(b, j). */
size_t lh_joints_mse_workspace_bytes(int b, int j);
int lh_joints_mse(const float* pred, const float* target, const float* weight, int b, int j, int hw, int topk, float* loss,
                  float* joint_loss, float* grad, const float* grad_scale, void* workspace, void* stream);
/* get_max_preds: src/utils/loss.py:327-355 (+ the x4 of src/utils/method.py:157,176-178 via
 * `scale`).  heatmaps fp32 NCHW [b*j][h*w] -> preds fp32 [b*j][2], maxvals fp32 [b*j],
 * idx int32 [b*j] (first-occurrence arg-max, NaN counts as maximum). */
int lh_heatmap_argmax(const float* heatmaps, int bj, int h, int w, float scale, float* preds,
                      float* maxvals, int* idx, void* stream);
/* Opt-in quarter-pixel refinement of lh_heatmap_argmax's result (NOT in the reference: its config carries the unused
 * switch TEST.POST_PROCESS, src/modeling/simplebaseline/config.py:109; this is the published SimpleBaseline rule
 * coord += 0.25 * sign(hm[+1] - hm[-1]) per axis for peaks strictly inside the map).  idx / maxvals / preds are
 * lh_heatmap_argmax's outputs (same scale); preds is updated in place. */
/* Opt-in soft-arg-max decode (the project brief names it; the reference decodes with the hard arg-max above, so this is an
 * extension without a reference oracle): preds[b*j] = sum_p softmax(beta * hm)[p] * (x_p, y_p) * scale. */
int lh_heatmap_soft_argmax(const float* heatmaps, int bj, int h, int w, float beta, float scale, float* preds,
                           void* stream);
int lh_heatmap_refine(const float* heatmaps, const int* idx, const float* maxvals, int bj, int h, int w,
                      float scale, float* preds, void* stream);
/* Integral-regression coordinate loss (Sun et al. 2018; an opt-in extension without a reference oracle): the L1 distance between
 * lh_heatmap_soft_argmax's expectation and the ground-truth joint, in input pixels, and its gradient through the softmax.
 * heatmaps / grad fp32 [b*j][h*w], joints fp32 read at joints[n * jstride + {0, 1}], weight fp32 [b*j] or NULL (ones), preds
 * fp32 [b*j][2], joint_loss optional fp32 [b*j], loss a device scalar, grad optional, grad_scale an optional device scalar read
 * on the device like lh_mse_heatmap's.  Per plane n, x_p = p % w, y_p = p / w:
 *   e_p = expf(beta * (hm_p - max hm)) in fp32; S0 = sum e_p, sum e_p x_p, sum e_p y_p in fp64 in a fixed order;
 *   ex = sum e_p x_p / S0, ey likewise (fp64); preds[n] = ((float)ex * scale, (float)ey * scale): lh_heatmap_soft_argmax's bits;
 *   r = preds[n] - joints[n] (fp32), s = sgn(r) per axis with sgn(0) = 0; joint_loss[n] = wgt_n * (|rx| + |ry|);
 *   loss_c = lambda * sum_n joint_loss[n] / (2*b*j), folded in fp64 in plane order by one small launch; *loss = loss_c, or
 *   *loss += loss_c when add_to_loss; the first 4 bytes of the workspace receive loss_c alone (fp32) either way;
 *   g_p = (e_p * k_n) * (float)((x_p - ex) * sx + (y_p - ey) * sy), the bracket in fp64,
 *   k_n = (float)(gs * lambda * wgt_n * scale * beta / (2*b*j) / S0), gs = grad_scale ? *grad_scale : 1;
 *   grad_p = g_p, or grad_p += g_p when add_to_grad.  A plane of weight 0 gets exactly 0.f (add_to_grad: it is not touched).
 * One workgroup per plane with the plane in LDS (read from memory once), 16-byte accesses on grad, no atomics: two calls give
 * the same bits.  Supported for h * w <= 96 * 96, h * w % 4 == 0, heatmaps / grad / workspace 16-byte aligned, beta > 0, finite
 * beta / scale / lambda (LH_ERR_ARG otherwise, before any launch); workspace >= lh_integral_l1_workspace_bytes(b, j). */
size_t lh_integral_l1_workspace_bytes(int b, int j);
int lh_integral_l1(const float* heatmaps, const float* joints, int jstride, const float* weight, int b, int j, int h, int w,
                   float beta, float scale, float lambda, float* preds, float* joint_loss, float* loss, int add_to_loss,
                   float* grad, int add_to_grad, const float* grad_scale, void* workspace, void* stream);
/* Opt-in DARK decode (Zhang et al. 2020: the published get_final_preds -> gaussian_blur -> taylor chain; NOT in the
 * reference), the sibling of lh_heatmap_refine: idx / maxvals / preds are the outputs of lh_heatmap_argmax or
 * lh_heatmap_flip_merge at the same `scale`; preds is updated in place, the heat-maps are only read.  Per plane, in fp32:
 *   skip     preds stays as it is unless maxvals > 0 and the peak (px, py) satisfies 1 < px < w-2 && 1 < py < h-2;
 *   blur     B = the plane under a separable, zero-padded Gaussian of blur_kernel taps g[t] = exp(-(t-c)^2 / (2 s^2)) / sum,
 *            c = (k-1)/2, s = 0.3*((k-1)*0.5 - 1) + 0.8 (cv2.getGaussianKernel's formula; evaluated on the host in fp64 and
 *            rounded to fp32); rows first, then columns, the taps accumulated in index order;
 *   log      C = log(max(B * (maxval / max(B)), 1e-10f)), max(B) over the whole blurred plane;
 *   taylor   dx = 0.5(C[py][px+1] - C[py][px-1]), dxx = 0.25(C[py][px+2] - 2C[py][px] + C[py][px-2]), dy / dyy likewise,
 *            dxy = 0.25(C[py+1][px+1] - C[py-1][px+1] - C[py+1][px-1] + C[py-1][px-1]), det = dxx*dyy - dxy^2;
 *            preds = ((px, py) - H^-1 (dx, dy)) * scale when det != 0 and both offsets are finite, unchanged otherwise.
 * The finiteness guard is this project's; OpenCV's fixed tap tables for kernels <= 7 are not reproduced (the formula above
 * is used for every size).  One workgroup per plane with the plane in LDS, no atomics: two calls give the same bits.
 * Supported for h * w <= 96 * 96 and blur_kernel odd in 3..17 (LH_ERR_ARG otherwise, before any launch). */
int lh_heatmap_dark(const float* heatmaps, const int* idx, const float* maxvals, int bj, int h, int w, int blur_kernel,
                    float scale, float* preds, void* stream);
/* Flip test's flip-back and merge (SimpleBaseline's flip_back + SHIFT_HEATMAP + average, TEST.FLIP_TEST of the reference's
 * configs) followed by lh_heatmap_argmax's decode, in one launch.  a = heat-maps of the plain input, m = those of the
 * horizontally mirrored input, fp32 [b*j][h][w]; f[y][x] = m[y][w-x] for x >= 1 and f[y][0] = m[y][w-1] when `shift`,
 * else f[y][x] = m[y][w-1-x]; merged = (a + f) * 0.5f.  preds / maxvals / idx (idx may be NULL) as lh_heatmap_argmax on
 * merged.  merged may alias a (the same pointer); it must not overlap m. */
int lh_heatmap_flip_merge(const float* a, const float* m, int bj, int h, int w, int shift, float scale, float* merged,
                          float* preds, float* maxvals, int* idx, void* stream);

/* Validation metrics of Runner.run (src/utils/method.py:243-250) on the device: per sample, wrong[b] = number of
 * joints with error / bbox-diagonal(gt) > T (PCK_2d_loss 'proportion', src/utils/loss.py:116-148) and epe[b] = sum of
 * the errors of joints 1..J-2 (EPE_train's joint range, src/utils/loss.py:50-67).  pred fp32 [b][j][2],
 * gt fp32 [b][j][gt_stride]. */
int lh_keypoint_metrics(const float* pred, const float* gt, int gt_stride, int b, int j, float T, int* wrong,
                        float* epe, void* stream);

/* ------------------------------------------------------------------ optimiser
 * torch.optim.Adam(lr, betas, eps, weight_decay=0).step(): src/tools/train.py:45-48,
 * src/utils/method.py:183.  One launch over a flat fp32 arena (plus a one-thread
 * tick kernel).  hyper (device, fp64[4]) = { lr, beta1, beta2, eps }; step (device int32) is
 * incremented on the device, so a captured hipGraph replays correctly; derived (device fp32[8])
 * is scratch for the bias-corrected step size evaluated in fp64 like the reference's Python. */
int lh_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long numel,
                 const double* hyper, int* step, float* derived, float grad_scale, void* stream);
/* The two halves of lh_adam_step, for an update applied SLICE BY SLICE (torch.optim.Adam's update is elementwise, so the
 * result is bit-identical to one lh_adam_step over the whole range): lh_adam_tick once per iteration (step += 1,
 * derived = bias-corrected step size ...), then lh_adam_apply per slice -- pointers advanced to the slice, which must
 * start on a 16-byte boundary. */
int lh_adam_tick(const double* hyper, int* step, float* derived, void* stream);
int lh_adam_apply(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long numel, const float* derived,
                  float grad_scale, void* stream);

/* Dynamic loss scaling (torch.amp.GradScaler + optimizer.step()) decided on the device, so that it lives inside a captured
 * step.  Per step, in this order on one stream:
 *   lh_amp_check           partial[k] (device int32[lh_amp_check_blocks()]) = 1 where workgroup k saw an inf / NaN in the RAW
 *                          gradient (before unscaling); every slot is rewritten at every call.  grad 16-byte aligned.
 *   lh_amp_update          found_inf = OR of partial; inv = extra / scale (fp64, rounded to fp32); skipped += found_inf; then
 *                          torch._amp_update_scale_ on scale (fp32) / growth_tracker (int32) with amp_hyper (device fp64[3]) =
 *                          { growth_factor, backoff_factor, growth_interval }; only when found_inf == 0 the tick of
 *                          lh_adam_tick (step += 1, derived).
 *   lh_adam_apply_guarded  lh_adam_apply with grad_scale = *inv, returning before it touches memory when *found_inf. */
int lh_amp_check_blocks(void);
int lh_amp_check(const float* grad, long numel, int* partial, void* stream);
int lh_amp_update(const int* partial, const double* amp_hyper, float* scale, int* growth_tracker, int* found_inf, int* skipped,
                  float* inv, double extra, const double* hyper, int* step, float* derived, void* stream);
int lh_adam_apply_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long numel, const float* derived,
                          const int* found_inf, const float* inv, void* stream);

/* Bias gradient of the head's 1x1 convolution (pose_resnet.py:169-175; loss.backward()): out[c] = sum over n, h, w of an
 * NCHW fp32 gradient.  fp64 partials in a fixed order (deterministic).  workspace >= lh_channel_sum_workspace_bytes(c). */
size_t lh_channel_sum_workspace_bytes(int c);
int lh_channel_sum_nchw(const float* x, int n, int c, int hw, float* out, void* workspace, void* stream);

/* Bias gradient of a convolution / transposed convolution WITH bias inside the network (DECONV_WITH_BIAS:
 * src/modeling/simplebaseline/pose_resnet.py:149,227; what autograd's loss.backward() adds for nn.ConvTranspose2d(bias=True)):
 * out[ch] = sum over `pixels` rows of an NHWC gradient of the run precision, channels [0, c) of rows of pix_stride
 * elements (16-byte aligned rows).  fp64 partials in a fixed order (deterministic); same workspace size. */
int lh_channel_sum_nhwc(const void* x, long pixels, int c, int pix_stride, float* out, void* workspace, int dtype, void* stream);

/* PCK curve of pred_eval (src/utils/argparser.py:326-388) on the device: counts[t] += visible joints (gt[..][2] == 1) whose
 * error (pixel distance; divided by bb[sample] when bb != NULL, the 'pckb' mode) is < thr[t]; *nvis += visible joints;
 * diff_row[s] = sum of pixel errors over ALL joints of sample s.  float64 arithmetic like the NumPy original; counts /
 * nvis ACCUMULATE (zero them first) with integer atomics, so the result is exact and ranks can be summed by one small
 * all-reduce.  AUC = trapz(100*counts/nvis, thr) / trapz(1, thr) on the host (lighthand_amd.metrics.auc_from_counts). */
int lh_pck_curve(const float* pred, const float* gt, int gt_stride, const float* bb, int n, int j, const double* thr,
                 int nthr, unsigned long long* counts, unsigned long long* nvis, double* diff_row, void* stream);

/* ------------------------------------------------------------------ data-parallel gradient exchange
 * The reference trains on one device (no DistributedDataParallel anywhere: src/utils/comm.py:15-32 only queries rank /
 * world size for logging and checkpoint gating); the data-parallel path is this engine's addition.  One
 * communicator per process (= per GPU) over RCCL / xGMI: rank 0 creates a 128-byte id (lh_comm_unique_id) that the host
 * side hands to every rank (any channel: torch.distributed's store, a file); lh_comm_allreduce_sum sums one gradient
 * bucket in place across the ranks, asynchronously on `stream` (legal inside hipGraph capture).  dtype: LH_F32 for exact
 * sums, LH_BF16 for half the bytes per link.  The library binds to the RCCL already loaded in the process. */
typedef struct lh_comm lh_comm;
int lh_comm_unique_id(void* id128);
int lh_comm_init(lh_comm** comm, int rank, int nranks, const void* id128);
int lh_comm_allreduce_sum(lh_comm* comm, void* buf, size_t count, int dtype, void* stream);
/* The pieces of a DIRECT gradient exchange (reduce-scatter + all-gather with all seven xGMI peers at once, 2 x bytes / N
 * per link instead of a ring's 2 (N - 1) / N x bytes over one), all stream-ordered and capturable like the all-reduce, so that the whole
 * data-parallel step stays ONE hipGraph (parallel.LhComm.direct_sum_):
 *   lh_comm_alltoall            recv chunk r <- rank r's send chunk `rank` (grouped point-to-point exchange, `count` elements per chunk);
 *                               then lh_sum_chunks adds the N received chunks in RANK order -- every rank ends with the same bits;
 *   lh_comm_allgather           recv chunk r <- rank r's `count` elements (recv + rank * count == send: in place);
 *   lh_comm_reduce_scatter_sum  RCCL's own reduce-scatter (recv <- the sum of every rank's send chunk `rank`), for comparison.
 * lh_comm_size: the rank / rank count the communicator was created with. */
int lh_comm_reduce_scatter_sum(lh_comm* comm, const void* send, void* recv, size_t count, int dtype, void* stream);
int lh_comm_allgather(lh_comm* comm, const void* send, void* recv, size_t count, int dtype, void* stream);
int lh_comm_alltoall(lh_comm* comm, const void* send, void* recv, size_t count, int dtype, void* stream);
int lh_comm_size(const lh_comm* comm, int* rank, int* nranks);
int lh_comm_destroy(lh_comm* comm);

/* dst[i0][i1][i2][i3] = src[i0][i1][i2][i3], fp32, element strides on both sides (shape4 / strides are HOST arrays read at
 * call time).  The layout shuffles of a step that the reference leaves to tensor views: the stem weight and its gradient
 * between [O][3][k][k] (pose_resnet.py:151) and the padded NHWC4 staging, the head-gradient crop, bias padding. */
int lh_copy_strided_f32(float* dst, const float* src, const int* shape4, const long* dst_strides4, const long* src_strides4,
                        void* stream);


/* Staging of a gradient bucket that travels as bfloat16 (parallel.GradSync(compress="bf16"); the reference has no
 * multi-GPU path): to_f32 = 0 rounds the fp32 arena slice `f32` into the bf16 buffer `b16` (nearest even),
 * to_f32 = 1 widens `b16` back into `f32`.  n elements, any alignment. */
int lh_cast_f32_bf16(float* f32, void* b16, long n, int to_f32, void* stream);

/* The local reduction of the DIRECT gradient exchange (parallel.GradSync(algo="direct"): all-to-all + this + all-gather = reduce-scatter
 * and all-gather with every xGMI peer at once): out[i] = sum over r < rows of in[r * len + i], accumulated in fp32 in row
 * (= rank) order and rounded once; dtype LH_F32 or LH_BF16; `out` may be the first row of `in`. */
int lh_sum_chunks(const void* in, void* out, int rows, long len, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTHAND_HIP_H */
