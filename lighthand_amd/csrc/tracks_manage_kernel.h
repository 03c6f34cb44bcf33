// Device side of lh_tracks_manage (tracks_manage.hip): track management of the tracked top-down step, one launch behind
// lh_keypoints_to_boxes / lh_keypoints_to_rois and in front of lh_one_euro: duplicate tracks are suppressed (greedy NMS over the live
// slots of a frame), slots that stay lost expire, and a detector's boxes that no kept track covers seed the frame's free slots.  The
// rule is stated in include/lighthand_hip.h and restated in numpy by lighthand_amd/topdown.py (manage_tracks_host); all arithmetic is
// fp32 in the order written (-ffp-contract=off), with no division and no sqrtf, so every decision is the host's bit for bit.
// (A mode of frames_crop_kernel<float>, as lh_roi_perturb's: the resource tables admit no new kernel symbol.  The launch is its own:
// one workgroup of ONE wave per frame and dynamic LDS sized for this call's slots and detections, so the crop's launches pay nothing.)
//
// The frame's slots and valid detections are compacted into LDS in ascending index (ballot + population count, so the order does not
// depend on timing), ranked by counting, and the two greedy walks run over LDS with the 64 lanes testing one candidate against 64
// earlier winners at a time.  Every global word has one writer, in the last pass: no atomics, no dependence on the order of the
// workgroups.
#pragma once
#include "common.h"

#define TM_MAX 1024                                                // slots, and detections, of one launch: 16-bit indices, 59 KB of LDS
#define TM_LIVE 1
#define TM_KEPT 2

struct tm_box { float x0, y0, x1, y1; };

// intersection over the smaller area > t, as comparisons and products: min / max by comparison, so the host's np.where is the same rule
__device__ __forceinline__ bool tm_over(const tm_box a, const tm_box b, float t) {
    const float ix1 = a.x1 < b.x1 ? a.x1 : b.x1, ix0 = a.x0 > b.x0 ? a.x0 : b.x0;
    const float iy1 = a.y1 < b.y1 ? a.y1 : b.y1, iy0 = a.y0 > b.y0 ? a.y0 : b.y0;
    const float iw = ix1 - ix0, ih = iy1 - iy0;
    if (!(iw > 0.f && ih > 0.f)) return false;
    const float aa = (a.x1 - a.x0) * (a.y1 - a.y0), ab = (b.x1 - b.x0) * (b.y1 - b.y0);
    const float sm = aa < ab ? aa : ab;
    return iw * ih > t * sm;
}

// the position of the first of list[0..n) (indices into box[]) that overlaps a, or -1: 64 entries per step, the same answer in every lane
__device__ __forceinline__ int tm_first_hit(const tm_box a, const tm_box* box, const unsigned short* list, int n, float t, int lane) {
    for (int base = 0; base < n; base += 64) {
        const int q = base + lane;
        const bool h = q < n && tm_over(a, box[list[q]], t);
        const unsigned long long mask = __ballot(h);
        if (mask) return base + __ffsll((long long)mask) - 1;
    }
    return -1;
}

// What lh_tracks_manage passes (CropArgs.tm): its arguments under their names in include/lighthand_hip.h.
struct TracksArgs {
    const float *preds, *maxvals, *det_boxes, *det_score;
    const int *src_frame, *frame_index, *det_frame;
    int b, j, n_frames, k, max_lost;
    float min_score, min_side, dup_overlap, match_overlap, det_min_score;
    float *next_boxes, *next_rot;
    int *lost, *lost_count, *dup_of, *seeded, *det_state;
};

// The LDS of one launch, carved from the dynamic block in this order (16-byte records first): bp = b and kp = k rounded up to 8.
__host__ __device__ inline size_t tm_lds_bytes(int b, int k) {
    const size_t bp = (size_t)(b + 7) / 8 * 8, kp = (size_t)(k + 7) / 8 * 8;
    return bp * (16 + 4 + 2 * 6 + 1) + kp * (16 + 4 + 2 * 3);
}

__device__ __forceinline__ void tracks_manage_frame(const TracksArgs& a, unsigned char* lds) {
    const float *preds = a.preds, *maxvals = a.maxvals, *det_boxes = a.det_boxes, *det_score = a.det_score;
    const int *src_frame = a.src_frame, *frame_index = a.frame_index, *det_frame = a.det_frame;
    const int b = a.b, j = a.j, n_frames = a.n_frames, K = a.k, max_lost = a.max_lost;
    const float min_score = a.min_score, min_side = a.min_side, dup_overlap = a.dup_overlap, match_overlap = a.match_overlap;
    const float det_min_score = a.det_min_score;
    float *next_boxes = a.next_boxes, *next_rot = a.next_rot;
    int *lost = a.lost, *lost_count = a.lost_count, *dup_of = a.dup_of, *seeded = a.seeded, *det_state = a.det_state;
    const int bp = (b + 7) / 8 * 8, kp = (K + 7) / 8 * 8;
    tm_box* s_kb = reinterpret_cast<tm_box*>(lds);                 // a member slot's keypoint bounds
    tm_box* s_db = s_kb + bp;                                      // a valid detection's box
    float* s_score = reinterpret_cast<float*>(s_db + kp);
    float* s_dscore = s_score + bp;
    unsigned short* s_slot = reinterpret_cast<unsigned short*>(s_dscore + kp);      // member -> slot
    unsigned short* s_order = s_slot + bp;                         // rank -> member (live ones)
    unsigned short* s_kept = s_order + bp;
    unsigned short* s_free = s_kept + bp;
    short* s_dup = reinterpret_cast<short*>(s_free + bp);          // member -> the kept member it duplicates, or -1
    short* s_seed = s_dup + bp;                                    // member -> the detection it takes, or -1
    unsigned short* s_didx = reinterpret_cast<unsigned short*>(s_seed + bp);        // valid detection -> entry of the list
    unsigned short* s_dorder = s_didx + kp;                        // rank -> valid detection
    unsigned short* s_dacc = s_dorder + kp;
    unsigned char* s_flag = reinterpret_cast<unsigned char*>(s_dacc + kp);
    const int f = blockIdx.x, lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;

    // 1. the frame's slots and its valid detections, in ascending index
    int nm = 0, nd = 0;
    for (int base = 0; base < b; base += 64) {
        const int i = base + lane;
        const bool mine = i < b && frame_index[i] == f;
        const unsigned long long mask = __ballot(mine);
        if (mine) s_slot[nm + __popcll(mask & below)] = (unsigned short)i;
        nm += __popcll(mask);
    }
    for (int base = 0; base < K; base += 64) {
        const int d = base + lane;
        bool valid = false;
        if (d < K) {
            const int df = det_frame[d];
            const bool in_range = df >= 0 && df < n_frames;
            if (df == f) {
                const float x0 = det_boxes[d * 4], y0 = det_boxes[d * 4 + 1], x1 = det_boxes[d * 4 + 2], y1 = det_boxes[d * 4 + 3];
                const float sc = det_score[d];
                valid = isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && x1 > x0 && y1 > y0 && isfinite(sc) && sc >= det_min_score;
            }
            if ((df == f && !valid) || (!in_range && f == 0)) det_state[d] = -1;       // an entry of no frame is workgroup 0's to mark
        }
        const unsigned long long mask = __ballot(valid);
        if (valid) s_didx[nd + __popcll(mask & below)] = (unsigned short)d;
        nd += __popcll(mask);
    }
    __syncthreads();

    // 2. the records: kb and score exactly as keypoints_to_boxes_kernel walks the joints
    int nl = 0;
    for (int base = 0; base < nm; base += 64) {
        const int m = base + lane;
        bool live = false;
        if (m < nm) {
            const int i = s_slot[m];
            float lo_x = 0.f, lo_y = 0.f, hi_x = 0.f, hi_y = 0.f, sum = 0.f;
            int n = 0;
            for (int k = 0; k < j; ++k) {
                const float v = maxvals[(long)i * j + k];
                if (!(v >= min_score)) continue;
                const float x = preds[((long)i * j + k) * 2], y = preds[((long)i * j + k) * 2 + 1];
                if (n == 0) { lo_x = hi_x = x; lo_y = hi_y = y; }
                lo_x = x < lo_x ? x : lo_x; hi_x = x > hi_x ? x : hi_x;
                lo_y = y < lo_y ? y : lo_y; hi_y = y > hi_y ? y : hi_y;
                sum = sum + v;
                ++n;
            }
            if (hi_x - lo_x < min_side) { const float c = (lo_x + hi_x) * 0.5f; lo_x = c - min_side * 0.5f; hi_x = c + min_side * 0.5f; }
            if (hi_y - lo_y < min_side) { const float c = (lo_y + hi_y) * 0.5f; lo_y = c - min_side * 0.5f; hi_y = c + min_side * 0.5f; }
            live = lost[i] == 0;
            s_kb[m] = tm_box{lo_x, lo_y, hi_x, hi_y};
            s_score[m] = sum;
            s_flag[m] = live ? TM_LIVE : 0;
            s_dup[m] = -1;
            s_seed[m] = -1;
        }
        nl += __popcll(__ballot(live));
    }
    for (int e = lane; e < nd; e += 64) {
        const int d = s_didx[e];
        s_db[e] = tm_box{det_boxes[d * 4], det_boxes[d * 4 + 1], det_boxes[d * 4 + 2], det_boxes[d * 4 + 3]};
        s_dscore[e] = det_score[d];
    }
    __syncthreads();

    // 3. ranks by counting: descending score, ties to the lower index (members and detections are stored in ascending index)
    for (int m = lane; m < nm; m += 64) {
        if (!(s_flag[m] & TM_LIVE)) continue;
        const float sc = s_score[m];
        int rank = 0;
        for (int k = 0; k < nm; ++k) rank += ((s_flag[k] & TM_LIVE) && (s_score[k] > sc || (s_score[k] == sc && k < m))) ? 1 : 0;
        s_order[rank] = (unsigned short)m;
    }
    for (int e = lane; e < nd; e += 64) {
        const float sc = s_dscore[e];
        int rank = 0;
        for (int k = 0; k < nd; ++k) rank += (s_dscore[k] > sc || (s_dscore[k] == sc && k < e)) ? 1 : 0;
        s_dorder[rank] = (unsigned short)e;
    }
    __syncthreads();

    // 4. duplicate tracks: greedy NMS in rank order; a candidate is tested against the kept list 64 entries at a time
    int nk = 0;
    for (int r = 0; r < nl; ++r) {
        const int c = s_order[r];
        const int hit = tm_first_hit(s_kb[c], s_kb, s_kept, nk, dup_overlap, lane);
        if (lane == 0) {
            if (hit < 0) { s_kept[nk] = (unsigned short)c; s_flag[c] = TM_LIVE | TM_KEPT; }
            else s_dup[c] = (short)s_kept[hit];
        }
        nk += hit < 0 ? 1 : 0;
        __syncthreads();
    }

    // 5. the free slots: every member that was not kept, in ascending index
    int nfree = 0;
    for (int base = 0; base < nm; base += 64) {
        const int m = base + lane;
        const bool fr = m < nm && !(s_flag[m] & TM_KEPT);
        const unsigned long long mask = __ballot(fr);
        if (fr) s_free[nfree + __popcll(mask & below)] = (unsigned short)m;
        nfree += __popcll(mask);
    }
    __syncthreads();

    // 6. detections in rank order: covered by a kept track, a repeat of an accepted detection, no room, or a seed
    int na = 0;
    for (int r = 0; r < nd; ++r) {
        const int e = s_dorder[r];
        const tm_box a = s_db[e];
        int state;
        bool take = false;
        if (tm_first_hit(a, s_kb, s_kept, nk, match_overlap, lane) >= 0) state = -2;
        else if (tm_first_hit(a, s_db, s_dacc, na, match_overlap, lane) >= 0) state = -3;
        else if (na >= nfree) state = -4;
        else { take = true; state = s_slot[s_free[na]]; }
        if (lane == 0) {
            if (take) { s_seed[s_free[na]] = (short)e; s_dacc[na] = (unsigned short)e; }
            det_state[s_didx[e]] = state;
        }
        na += take ? 1 : 0;                                          // the accepted detections and the free slots taken count alike
        __syncthreads();
    }

    // 7. expiry and write-out: one writer per word
    for (int m = lane; m < nm; m += 64) {
        const int i = s_slot[m], dup = s_dup[m], e = s_seed[m];
        bool empty = false;
        int count = 0;
        if (s_flag[m] & TM_KEPT) {
        } else if (dup >= 0) {
            lost[i] = 1;
            empty = true;
        } else if (src_frame[i] >= 0) {
            const int c = lost_count[i];
            count = c < (1 << 30) ? c + 1 : (1 << 30);
            if (max_lost > 0 && count >= max_lost) { empty = true; count = 0; }
        }
        dup_of[i] = dup >= 0 ? (int)s_slot[dup] : -1;
        seeded[i] = e >= 0 ? (int)s_didx[e] : -1;
        if (e >= 0) {
            const tm_box d = s_db[e];
            next_boxes[i * 4] = d.x0; next_boxes[i * 4 + 1] = d.y0; next_boxes[i * 4 + 2] = d.x1; next_boxes[i * 4 + 3] = d.y1;
            if (next_rot) { next_rot[i * 2] = 1.f; next_rot[i * 2 + 1] = 0.f; }
            count = 0;
        } else if (empty) {
            next_boxes[i * 4] = 0.f; next_boxes[i * 4 + 1] = 0.f; next_boxes[i * 4 + 2] = 0.f; next_boxes[i * 4 + 3] = 0.f;
        }
        lost_count[i] = count;
    }
}
