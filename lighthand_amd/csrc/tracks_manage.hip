// lh_tracks_manage: track management of the tracked top-down step (the rule and the device code: tracks_manage_kernel.h).  The entry
// checks its arguments and launches the mode of frames_crop_kernel<float> that carries it, through frames_crop.hip's launcher.
#include "frames_crop_kernel.h"

extern "C" int lh_tracks_manage(const float* preds_dev, const float* maxvals_dev, const int* src_frame_dev, const int* frame_index_dev, int b,
                                int j, int n_frames, const float* det_boxes_dev, const int* det_frame_dev, const float* det_score_dev, int k,
                                float track_min_score, float track_min_side, float dup_overlap, float match_overlap, float det_min_score,
                                int max_lost, float* next_boxes_dev, float* next_rot_dev, int* lost_dev, int* lost_count_dev, int* dup_of_dev,
                                int* seeded_dev, int* det_state_dev, void* stream) {
    LH_REQUIRE(b >= 1 && b <= TM_MAX && k >= 1 && k <= TM_MAX, "lh_tracks_manage: 1 <= b <= %d slots and 1 <= k <= %d detections, got %d and %d",
               TM_MAX, TM_MAX, b, k);
    LH_REQUIRE(preds_dev && maxvals_dev && src_frame_dev && frame_index_dev && det_boxes_dev && det_frame_dev && det_score_dev && next_boxes_dev
               && lost_dev && lost_count_dev && dup_of_dev && seeded_dev && det_state_dev, "lh_tracks_manage: null pointer (only next_rot may be)");
    LH_REQUIRE(j > 0 && (long)b * j < (1L << 30) && n_frames > 0, "lh_tracks_manage: j and n_frames must be > 0, got %d and %d", j, n_frames);
    LH_REQUIRE(track_min_score == track_min_score && track_min_score >= -3.0e38f && track_min_score <= 3.0e38f && track_min_side >= 0.f
               && track_min_side <= 3.0e38f && dup_overlap >= 0.f && dup_overlap <= 3.0e38f && match_overlap >= 0.f && match_overlap <= 3.0e38f
               && det_min_score >= 0.f && det_min_score <= 3.0e38f,
               "lh_tracks_manage: thresholds must be finite, and all but track_min_score >= 0");
    LH_REQUIRE(max_lost >= 0, "lh_tracks_manage: max_lost must be >= 0, got %d", max_lost);
    CropArgs a = {};
    a.op = LH_CROP_TRACKS_MANAGE;
    a.tm = TracksArgs{preds_dev, maxvals_dev, det_boxes_dev, det_score_dev, src_frame_dev, frame_index_dev, det_frame_dev, b, j, n_frames, k, max_lost,
                      track_min_score, track_min_side, dup_overlap, match_overlap, det_min_score, next_boxes_dev, next_rot_dev, lost_dev,
                      lost_count_dev, dup_of_dev, seeded_dev, det_state_dev};
    lh_frames_crop_launch_f32(a, n_frames, 64, tm_lds_bytes(b, k), stream);      // one workgroup of one wave per frame
    LH_LAUNCH_CHECK("tracks_manage launch");
    return LH_OK;
}
