// lh_draw_hands: the skeleton overlay of the tracked top-down step (the rule and the device code: draw_hands_kernel.h).  The entry checks
// its arguments and launches the mode of frames_crop_kernel<float> that carries it, through frames_crop.hip's launcher; the frames'
// layout passes the checks of the surfaces crop entry (lh_frames_layout_args).
#include "frames_crop_kernel.h"

extern "C" int lh_draw_hands(unsigned char* frames, long frame_stride, const long long* surface_table_dev, const lh_frames_layout* layout,
                             int n_frames, int hs, int ws, const float* preds_dev, const float* maxvals_dev, const int* src_frame_dev,
                             const int* lost_dev, const float* mat_dev, const float* boxes_dev, int b, int j, int crop_h, int crop_w,
                             const int* parents_dev, const int* group_dev, const float* palette_dev, int n_groups, float min_score,
                             float line_radius, float joint_radius, float by_size, float opacity, int draw_roi, void* stream) {
    const char* who = "lh_draw_hands";
    LH_REQUIRE(frames || surface_table_dev, "%s: no frame source (frames and surface_table_dev are both null)", who);
    LH_REQUIRE(!(frames && surface_table_dev), "%s: two frame sources (pass frames or surface_table_dev, not both)", who);
    LH_REQUIRE(layout && preds_dev && maxvals_dev && src_frame_dev && parents_dev && group_dev && palette_dev,
               "%s: null pointer (only lost, mat, and boxes without by_size, may be)", who);
    LH_REQUIRE(!surface_table_dev || ((uintptr_t)surface_table_dev & 7) == 0, "%s: surface_table_dev must be 8-byte aligned", who);
    LH_REQUIRE(b >= 1 && b <= DRAW_MAX, "%s: 1 <= b <= %d slots, got %d", who, DRAW_MAX, b);
    LH_REQUIRE(j > 0 && (long)b * j < (1L << 28) && n_groups > 0 && n_groups < (1 << 20) && n_frames > 0 && hs > 0 && ws > 0 && crop_h > 0 && crop_w > 0,
               "%s: j, n_groups, n_frames, hs, ws, crop_h and crop_w must be > 0, got %d, %d, %d, %d, %d, %d and %d", who, j, n_groups, n_frames, hs,
               ws, crop_h, crop_w);
    LH_REQUIRE(line_radius >= 0.f && line_radius <= 3.0e38f && joint_radius >= 0.f && joint_radius <= 3.0e38f && by_size >= 0.f && by_size <= 3.0e38f,
               "%s: line_radius, joint_radius and by_size must be finite and >= 0", who);
    LH_REQUIRE(min_score >= -3.0e38f && min_score <= 3.0e38f, "%s: min_score must be finite", who);
    LH_REQUIRE(opacity >= 0.f && opacity <= 1.f, "%s: opacity must be in 0..1", who);
    LH_REQUIRE(boxes_dev || by_size == 0.f, "%s: by_size needs boxes_dev", who);
    const void* const fr = frames;
    LH_REQUIRE(!fr || (fr != preds_dev && fr != maxvals_dev && fr != src_frame_dev && fr != lost_dev && fr != mat_dev && fr != boxes_dev
                       && fr != parents_dev && fr != group_dev && fr != palette_dev),
               "%s: the frames must be distinct from every input", who);
    LH_REQUIRE((const void*)palette_dev != (const void*)preds_dev && (const void*)palette_dev != (const void*)maxvals_dev,
               "%s: palette, preds and maxvals must be distinct", who);
    CropArgs a = {};
    a.op = LH_CROP_DRAW_HANDS;
    a.dst = frames; a.table = surface_table_dev;
    if (const int rc = lh_frames_layout_args(who, layout, hs, ws, frames, frame_stride, a)) return rc;
    a.n_frames = n_frames; a.hs = hs; a.ws = ws; a.h = crop_h; a.w = crop_w; a.n = b; a.j = j;
    a.src_frame = src_frame_dev; a.mat = mat_dev;
    a.dr = DrawArgs{preds_dev, maxvals_dev, boxes_dev, palette_dev, lost_dev, parents_dev, group_dev, n_groups, draw_roi != 0, min_score,
                    line_radius, joint_radius, by_size, opacity};
    lh_frames_crop_launch_f32(a, b * DRAW_WGS, 256, draw_lds_bytes(b), stream);
    LH_LAUNCH_CHECK("draw_hands launch");
    return LH_OK;
}
