// Host side of the frame crop: the five crop entries, one launcher, and the two entries of training on frames that run as modes of
// the crop kernel's fp32 instantiation.  This is the one translation unit that instantiates frames_crop_kernel (frames_crop_kernel.h).
#include "frames_crop_kernel.h"

// What every crop entry is called with, whatever its frames are.
struct CropCall {
    const char* who;                                              // the entry's name in the error texts
    void* out;
    int b, n_frames, hs, ws, h, w, pad, wp;
    const float *mean3, *std3, *mat_dev;
    const int* src_frame_dev;
    int max_taps;
    bool jitter;                                                  // ColorJitter: factors, order and workspace are then all needed
    const float* factors;
    const int* order;
    void* workspace;                                              // the grey-mean partials (lh_frames_crop_jitter_workspace_bytes)
    int dtype;
    void* stream;
};

// The checks the entries share.  source_ok: the entry's own pointer (its frame buffer, or its layout).  One slot's pixels and one frame's
// bytes are 32-bit quantities (frame_fits, ``what`` its words in the error text); the frame BUFFER is indexed with long (64 frames of
// 1080p pass 2^31).
static int crop_check(const CropCall& c, bool source_ok, bool frame_fits, const char* what) {
    const char* who = c.who;
    LH_REQUIRE(source_ok && c.out && c.mean3 && c.std3 && c.mat_dev && c.src_frame_dev && c.b > 0 && c.b <= 65535 && c.n_frames > 0 && c.hs > 0
               && c.ws > 0 && c.h > 0 && c.w > 0 && c.pad >= 0 && c.wp >= c.w + 2 * c.pad, "%s: bad arguments", who);
    LH_REQUIRE(!c.jitter || (c.factors && c.order && c.workspace), "%s: bad arguments (factors_dev, order_dev or workspace is null)", who);
    LH_REQUIRE(!c.jitter || ((uintptr_t)c.workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    LH_REQUIRE(c.max_taps >= 1 && c.max_taps <= 8, "%s: max_taps must be 1..8, not %d", who, c.max_taps);
    LH_REQUIRE(lh_dtype_size(c.dtype) > 0, "%s: unsupported dtype %d", who, c.dtype);
    LH_REQUIRE(((uintptr_t)c.out & 7) == 0, "%s: out must be 8-byte aligned", who);
    LH_REQUIRE((long)(c.h + 2 * c.pad) * c.wp < (1L << 29) && frame_fits, "%s: %s too large for 32-bit pixel indices", who, what);
    return LH_OK;
}

// The kernel's arguments but for where the frames are (src / table, format and the layout's fields: the entry's own).
static CropArgs crop_args(const CropCall& c) {
    CropArgs a = {};
    a.dst = c.out; a.mat = c.mat_dev; a.src_frame = c.src_frame_dev;
    a.n_frames = c.n_frames; a.hs = c.hs; a.ws = c.ws; a.h = c.h; a.w = c.w; a.pad = c.pad; a.hp = c.h + 2 * c.pad; a.wp = c.wp;
    a.max_taps = c.max_taps; a.op = LH_CROP; a.jdtype = c.dtype;
    for (int ch = 0; ch < 3; ++ch) { a.mean[ch] = c.mean3[ch]; a.istd[ch] = 1.f / c.std3[ch]; }
    if (c.jitter) { a.jfactors = c.factors; a.jorder = c.order; a.jpartial = (double*)c.workspace; }
    return a;
}

// With ColorJitter the grey-mean launch goes first (grid (CJ_STRIPS, b)), then the crop (the apply mode: jfactors is set).  Both, and
// the surfaces entry's crop, are the fp32 instantiation's, which stores in a.jdtype; the other crops run their dtype's own.
static int crop_enqueue(const CropCall& c, CropArgs a, const char* grey_label, const char* label) {
    const dim3 grid(lh_grid((long)a.hp * a.wp, 1024), c.b);
    if (c.jitter) {
        a.op = LH_CROP_GREY_MEAN;                                 // the samples are fp32 whatever the crop's dtype is
        hipLaunchKernelGGL((frames_crop_kernel<float>), dim3(CJ_STRIPS, c.b), dim3(256), 0, (hipStream_t)c.stream, a);
        LH_LAUNCH_CHECK(grey_label);
        a.op = LH_CROP;
    }
    LH_DISPATCH_DTYPE(c.jitter || a.gen ? LH_F32 : c.dtype, T,
                      hipLaunchKernelGGL((frames_crop_kernel<T>), grid, dim3(256), 0, (hipStream_t)c.stream, a));
    LH_LAUNCH_CHECK(label);
    return LH_OK;
}

// What the NV12 entry adds to the RGB ones' arguments.
struct Nv12Layout {
    int pitch, uv_offset;
    long frame_stride;
    int siting;
    const float* csc12;
};

// The entries of one frame buffer: yuv = nullptr packed RGB frames, max_taps = 1 the plain crop.
static int frames_crop_launch(const CropCall& c, const unsigned char* frames_u8, const Nv12Layout* yuv = nullptr) {
    const char* who = c.who;
    const int hs = c.hs, ws = c.ws;
    if (const int rc = crop_check(c, frames_u8 != nullptr, yuv || (long)hs * ws * 3 < (1L << 31), "crop or frame")) return rc;
    CropArgs a = crop_args(c);
    a.src = frames_u8; a.format = yuv ? LH_FRAMES_NV12 : LH_FRAMES_RGB;
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
        for (int ch = 0; ch < 12; ++ch) LH_REQUIRE(yuv->csc12[ch] - yuv->csc12[ch] == 0.f, "%s: csc12[%d] is not finite", who, ch);
        a.pitch = yuv->pitch; a.uv_offset = yuv->uv_offset; a.frame_stride = yuv->frame_stride; a.siting = yuv->siting;
        for (int ch = 0; ch < 9; ++ch) a.k[ch] = yuv->csc12[ch];
        for (int ch = 0; ch < 3; ++ch) a.o[ch] = yuv->csc12[9 + ch];
    }
    return crop_enqueue(c, a, "frames_crop_jitter_to_nhwc4 grey-mean launch",
                        c.jitter ? "frames_crop_jitter_to_nhwc4 launch" : yuv ? "frames_crop_yuv_to_nhwc4 launch"
                        : c.max_taps > 1 ? "frames_crop_area_to_nhwc4 launch" : "frames_crop_to_nhwc4 launch");
}

extern "C" int lh_frames_crop_to_nhwc4(const unsigned char* frames_u8, void* out, int b, int n_frames, int hs, int ws, int h, int w, int pad,
                                       int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                                       int dtype, void* stream) {
    return frames_crop_launch({"lh_frames_crop_to_nhwc4", out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev, src_frame_dev, 1,
                               false, nullptr, nullptr, nullptr, dtype, stream}, frames_u8);
}

extern "C" int lh_frames_crop_area_to_nhwc4(const unsigned char* frames_u8, void* out, int b, int n_frames, int hs, int ws, int h, int w,
                                            int pad, int wp, const float* mean3, const float* std3, const float* mat_dev,
                                            const int* src_frame_dev, int max_taps, int dtype, void* stream) {
    return frames_crop_launch({"lh_frames_crop_area_to_nhwc4", out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev, src_frame_dev,
                               max_taps, false, nullptr, nullptr, nullptr, dtype, stream}, frames_u8);
}

extern "C" int lh_frames_crop_yuv_to_nhwc4(const unsigned char* frames_nv12, void* out, int b, int n_frames, int hs, int ws, int pitch,
                                           int uv_offset, long frame_stride, int chroma_siting, const float* csc12, int h, int w, int pad,
                                           int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                                           int max_taps, int dtype, void* stream) {
    const Nv12Layout yuv = {pitch, uv_offset, frame_stride, chroma_siting, csc12};
    return frames_crop_launch({"lh_frames_crop_yuv_to_nhwc4", out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev, src_frame_dev,
                               max_taps, false, nullptr, nullptr, nullptr, dtype, stream}, frames_nv12, &yuv);
}

extern "C" size_t lh_frames_crop_jitter_workspace_bytes(int b) { return b > 0 ? (size_t)b * CJ_STRIPS * sizeof(double) : 0; }

extern "C" int lh_frames_crop_jitter_to_nhwc4(const unsigned char* frames, void* out, int b, int n_frames, int hs, int ws, int pitch,
                                              int uv_offset, long frame_stride, int chroma_siting, const float* csc12, int h, int w, int pad,
                                              int wp, const float* mean3, const float* std3, const float* mat_dev, const int* src_frame_dev,
                                              int max_taps, const float* factors_dev, const int* order_dev, void* workspace, int dtype,
                                              void* stream) {
    const Nv12Layout yuv = {pitch, uv_offset, frame_stride, chroma_siting, csc12};
    return frames_crop_launch({"lh_frames_crop_jitter_to_nhwc4", out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev, src_frame_dev,
                               max_taps, true, factors_dev, order_dev, workspace, dtype, stream}, frames, csc12 ? &yuv : nullptr);
}

// Where the frames of a plane descriptor are: every check of ``layout`` for hs x ws frames (and of the buffer ``frames`` /
// ``frame_stride``, null: a surface table), and the fields of CropArgs the kernel finds a sample through -- format, pitch, siting, dsc,
// k, o, frame_stride.  Shared with lh_draw_hands (draw_hands.hip), which writes through the same descriptor.
int lh_frames_layout_args(const char* who, const lh_frames_layout* layout, int hs, int ws, const unsigned char* frames, long frame_stride,
                          CropArgs& a) {
    const int f = layout->format;
    LH_REQUIRE(f >= LH_FRAMES_FMT_RGB && f <= LH_FRAMES_FMT_P010, "%s: unknown format code %d", who, f);
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
        for (int ch = 0; ch < 12; ++ch) LH_REQUIRE(layout->csc12[ch] - layout->csc12[ch] == 0.f, "%s: csc12[%d] is not finite", who, ch);
        a.format = sb == 2 ? LH_FRAMES_420W : LH_FRAMES_420;
        a.pitch = (int)pitch; a.siting = layout->chroma_siting;
        a.dsc[0] = (int)c_pitch; a.dsc[1] = (int)cb; a.dsc[2] = (int)cr; a.dsc[3] = planar ? 1 : 2 * sb;
        for (int ch = 0; ch < 9; ++ch) a.k[ch] = layout->csc12[ch];
        for (int ch = 0; ch < 3; ++ch) a.o[ch] = layout->csc12[9 + ch];
        LH_REQUIRE(sb == 1 || !frames || (((uintptr_t)frames | (uintptr_t)frame_stride) & 1) == 0,
                   "%s: p010 samples are 16-bit: frames and frame_stride must be even", who);
    }
    LH_REQUIRE(need < (1L << 31), "%s: a frame of %ld bytes does not fit 32-bit byte indices", who, need);
    LH_REQUIRE(!frames || frame_stride >= need, "%s: frame_stride %ld is below the %ld bytes a frame's samples span", who, frame_stride, need);
    a.frame_stride = frames ? frame_stride : 0;
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ decoder surfaces, 4:2:0 flavours
// The entry of the surface table and the plane descriptor (the rules: frames_crop_kernel.h, above crop_texel and above the kernel's
// table load).  Every launch is the fp32 instantiation's, which stores in ``dtype``.  All of the layout is checked here, in front of
// any launch: the kernel trusts it.
extern "C" int lh_frames_crop_surfaces_to_nhwc4(const unsigned char* frames, void* out, long frame_stride, const long long* surface_table_dev,
                                                const lh_frames_layout* layout, int b, int n_frames, int hs, int ws, int h, int w,
                                                int pad, int wp, const float* mean3, const float* std3, const float* mat_dev,
                                                const int* src_frame_dev, int max_taps, const float* factors_dev, const int* order_dev,
                                                void* workspace, int dtype, void* stream) {
    const char* who = "lh_frames_crop_surfaces_to_nhwc4";
    const CropCall c = {who, out, b, n_frames, hs, ws, h, w, pad, wp, mean3, std3, mat_dev, src_frame_dev, max_taps,
                        factors_dev || order_dev || workspace, factors_dev, order_dev, workspace, dtype, stream};
    LH_REQUIRE(frames || surface_table_dev, "%s: no frame source (frames and surface_table_dev are both null)", who);
    LH_REQUIRE(!(frames && surface_table_dev), "%s: two frame sources (pass frames or surface_table_dev, not both)", who);
    if (const int rc = crop_check(c, layout != nullptr, true, "crop")) return rc;
    LH_REQUIRE(!surface_table_dev || ((uintptr_t)surface_table_dev & 7) == 0, "%s: surface_table_dev must be 8-byte aligned", who);
    CropArgs a = crop_args(c);
    a.src = frames; a.table = surface_table_dev; a.gen = 1;
    if (const int rc = lh_frames_layout_args(who, layout, hs, ws, frames, frame_stride, a)) return rc;
    return crop_enqueue(c, a, "frames_crop_surfaces_to_nhwc4 grey-mean launch", "frames_crop_surfaces_to_nhwc4 launch");
}

// ------------------------------------------------------------------------------------------------ training on frames: the two modes
void lh_frames_crop_launch_f32(const CropArgs& a, int grid, int block, size_t lds, void* stream) {
    hipLaunchKernelGGL((frames_crop_kernel<float>), dim3(grid), dim3(block), lds, (hipStream_t)stream, a);
}

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
