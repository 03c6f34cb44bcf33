// lh_rois_predict and lh_one_euro_gated: motion-aware tracking of the tracked top-down step (the rules and the device code:
// motion_kernel.h).  The entries check their arguments and launch the modes of frames_crop_kernel<float> that carry them, through
// frames_crop.hip's launcher.
#include "frames_crop_kernel.h"

extern "C" int lh_rois_predict(float* next_boxes_dev, const int* lost_dev, const int* src_frame_dev, const int* seeded_dev, const float* dt_dev,
                               int b, float cutoff, float lead, float max_shift, int coast, float* centre_dev, float* vel_dev, int* seen_dev,
                               int* coasted_dev, void* stream) {
    LH_REQUIRE(next_boxes_dev && lost_dev && src_frame_dev && dt_dev && centre_dev && vel_dev && seen_dev && coasted_dev,
               "lh_rois_predict: null pointer (only seeded may be)");
    LH_REQUIRE(b > 0 && b < (1 << 28), "lh_rois_predict: b must be > 0, got %d", b);
    LH_REQUIRE(cutoff > 0.f && cutoff <= 3.0e38f && lead >= 0.f && lead <= 3.0e38f && max_shift >= 0.f && max_shift <= 3.0e38f && coast >= 0,
               "lh_rois_predict: cutoff must be finite and > 0, lead, max_shift and coast finite and >= 0");
    LH_REQUIRE(centre_dev != vel_dev && centre_dev != next_boxes_dev && vel_dev != next_boxes_dev && seen_dev != coasted_dev,
               "lh_rois_predict: next_boxes and the state arrays must be distinct");
    CropArgs a = {};
    a.op = LH_CROP_ROIS_PREDICT;
    a.pr = PredictArgs{next_boxes_dev, lost_dev, src_frame_dev, seeded_dev, dt_dev, b, coast, cutoff, lead, max_shift, centre_dev, vel_dev,
                       seen_dev, coasted_dev};
    lh_frames_crop_launch_f32(a, (b + 63) / 64, 64, 0, stream);   // one thread per slot
    LH_LAUNCH_CHECK("rois_predict launch");
    return LH_OK;
}

extern "C" int lh_one_euro_gated(const float* x_dev, const float* maxvals_dev, const float* next_boxes_dev, const int* src_frame_dev,
                                 const int* lost_dev, const float* dt_dev, int b, int j, float min_cutoff, float beta, float d_cutoff,
                                 float gate_min_score, int by_size, float* xhat_dev, float* dxhat_dev, int* seen_j_dev, float* gap_dev,
                                 float* out_dev, void* stream) {
    LH_REQUIRE(x_dev && maxvals_dev && src_frame_dev && dt_dev && xhat_dev && dxhat_dev && seen_j_dev && gap_dev && out_dev && (next_boxes_dev || !by_size),
               "lh_one_euro_gated: null pointer (only lost may be, and next_boxes without by_size)");
    LH_REQUIRE(b > 0 && j > 0 && (long)b * j < (1L << 30), "lh_one_euro_gated: b and j must be > 0, got %d and %d", b, j);
    LH_REQUIRE(min_cutoff > 0.f && min_cutoff <= 3.0e38f && beta >= 0.f && beta <= 3.0e38f && d_cutoff > 0.f && d_cutoff <= 3.0e38f
               && gate_min_score >= -3.0e38f && gate_min_score <= 3.0e38f,
               "lh_one_euro_gated: min_cutoff and d_cutoff must be finite and > 0, beta finite and >= 0, gate_min_score finite");
    LH_REQUIRE(xhat_dev != x_dev && dxhat_dev != x_dev && xhat_dev != dxhat_dev && out_dev != xhat_dev && out_dev != dxhat_dev && gap_dev != xhat_dev
               && gap_dev != dxhat_dev && gap_dev != out_dev && gap_dev != x_dev, "lh_one_euro_gated: x, out and the state arrays must be distinct");
    CropArgs a = {};
    a.op = LH_CROP_ONE_EURO_GATED;
    a.og = GatedArgs{x_dev, maxvals_dev, next_boxes_dev, dt_dev, src_frame_dev, lost_dev, j, by_size != 0, min_cutoff, beta, d_cutoff,
                     gate_min_score, xhat_dev, dxhat_dev, gap_dev, out_dev, seen_j_dev};
    lh_frames_crop_launch_f32(a, b, 64, 0, stream);               // one workgroup of one wave per slot, as lh_one_euro's
    LH_LAUNCH_CHECK("one_euro_gated launch");
    return LH_OK;
}
