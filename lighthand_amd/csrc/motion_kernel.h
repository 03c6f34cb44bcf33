// Device side of lh_rois_predict and lh_one_euro_gated (motion.hip): motion-aware tracking of the tracked top-down step.  The rules are
// stated in include/lighthand_hip.h and restated in numpy by lighthand_amd/topdown.py (rois_predict_host, one_euro_gated_host); all
// arithmetic is fp32 in the order written (-ffp-contract=off), + - * /, fabsf, fminf / fmaxf and comparisons only, so the host takes
// every step bit for bit.  (Two modes of frames_crop_kernel<float>, as lh_tracks_manage's: the resource tables admit no new kernel
// symbol.  Each has a launch of its own -- workgroups of ONE wave, no dynamic LDS -- so the crop's launches pay nothing.)
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------ ROI velocity prediction and coasting
// lh_rois_predict edits next_boxes in place behind lh_keypoints_to_boxes / lh_keypoints_to_rois (and lh_tracks_manage): the next crop
// is taken where the hand will be, not where it was.  An oriented box's centre is a frame-coordinate point, so the same translation
// serves upright and oriented ROIs.  State per slot: centre (of the last box the hand was found in, moved along while coasting), vel
// (frame px / s, a low-passed finite difference of the centres: one_euro_kernel's derivative filter), seen, coasted.
// One thread per slot: every word has one writer, no atomics.
struct PredictArgs {
    float* next_boxes;
    const int *lost, *src_frame, *seeded;                          // seeded may be null
    const float* dt;
    int b, coast;
    float cutoff, lead, max_shift;
    float *centre, *vel;
    int *seen, *coasted;
};

__device__ __forceinline__ float predict_clamp(float s, float lim) { return fminf(fmaxf(s, -lim), lim); }

__device__ __forceinline__ void rois_predict_slot(const PredictArgs& a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.b) return;
    float* box = a.next_boxes + i * 4;
    const float x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    const float bw = x1 - x0, bh = y1 - y0;
    const float dt = a.dt[i];
    const bool okdt = dt > 0.f && isfinite(dt);
    // 1. reset: an empty slot, one a detection has just seeded, one track management has emptied.  The box is left alone.
    if (a.src_frame[i] < 0 || (a.seeded && a.seeded[i] >= 0) || !(bw > 0.f && bh > 0.f)) {
        a.seen[i] = 0; a.vel[i * 2] = 0.f; a.vel[i * 2 + 1] = 0.f; a.coasted[i] = 0;
        return;
    }
    const float lim = a.max_shift * fmaxf(bw, bh);
    const float vx = a.vel[i * 2], vy = a.vel[i * 2 + 1];
    // 2. lost: the box (which repeats the last one) coasts along the last velocity for up to `coast` replays, then the track is forgotten
    if (a.lost[i] != 0) {
        if (a.seen[i] != 0 && okdt && a.coasted[i] < a.coast) {
            const float sx = predict_clamp(vx * dt, lim), sy = predict_clamp(vy * dt, lim);
            box[0] = x0 + sx; box[1] = y0 + sy; box[2] = x1 + sx; box[3] = y1 + sy;
            a.centre[i * 2] += sx; a.centre[i * 2 + 1] += sy;
            a.coasted[i] += 1;
        } else {
            a.seen[i] = 0; a.vel[i * 2] = 0.f; a.vel[i * 2 + 1] = 0.f;
        }
        return;
    }
    // 3. found
    const float cx = (x0 + x1) * 0.5f, cy = (y0 + y1) * 0.5f;
    if (a.seen[i] == 0 || !okdt) {
        a.centre[i * 2] = cx; a.centre[i * 2 + 1] = cy;
        a.vel[i * 2] = 0.f; a.vel[i * 2 + 1] = 0.f;
        a.seen[i] = 1; a.coasted[i] = 0;
        return;
    }
    const float vmx = (cx - a.centre[i * 2]) / dt, vmy = (cy - a.centre[i * 2 + 1]) / dt;
    const float r = (6.2831855f * a.cutoff) * dt, al = r / (r + 1.f);
    const float nvx = al * vmx + (1.f - al) * vx, nvy = al * vmy + (1.f - al) * vy;
    a.centre[i * 2] = cx; a.centre[i * 2 + 1] = cy;
    a.coasted[i] = 0;
    if (!(isfinite(nvx) && isfinite(nvy))) {                      // (seen stays 1)
        a.vel[i * 2] = 0.f; a.vel[i * 2 + 1] = 0.f;
        return;
    }
    a.vel[i * 2] = nvx; a.vel[i * 2 + 1] = nvy;
    const float sx = predict_clamp((a.lead * nvx) * dt, lim), sy = predict_clamp((a.lead * nvy) * dt, lim);
    box[0] = x0 + sx; box[1] = y0 + sy; box[2] = x1 + sx; box[3] = y1 + sy;
}

// ------------------------------------------------------------------------------------------------ One-Euro, gated per joint
// lh_one_euro_gated is one_euro_kernel (roi_track.hip) with a confidence gate per joint and, with by_size, the speed that beta multiplies
// in hand sizes per second.  The launch shape is the same: one workgroup of 64 per slot, one thread per coordinate, strided when
// j * 2 > 64.  seen_j and gap are per JOINT but read by both of its coordinates' threads: every thread reads them before the barrier,
// and the joint's words are written behind it, by one thread per joint.  A joint that is gated out holds its filtered position and
// counts the seconds it has gone without an update (gap); on its return the update runs over T = gap + dt.  With the gate open
// (gate_min_score = -3.0e38f) and by_size = 0, T = 0 + dt = dt and every operation is one_euro_kernel's, in its order.
struct GatedArgs {
    const float *x, *maxvals, *next_boxes, *dt;
    const int *src_frame, *lost;                                   // lost may be null
    int j, by_size;
    float min_cutoff, beta, d_cutoff, gate_min_score;
    float *xhat, *dxhat, *gap, *out;
    int* seen_j;
};

__device__ __forceinline__ void one_euro_gated_slot(const GatedArgs& a) {
    const int slot = blockIdx.x, j = a.j, j2 = j * 2;
    const bool away = a.src_frame[slot] < 0 || (a.lost && a.lost[slot] != 0);
    const float dt = a.dt[slot];
    float size = 1.f;
    if (a.by_size) {
        const float* box = a.next_boxes + slot * 4;
        size = fmaxf(fmaxf(box[2] - box[0], box[3] - box[1]), 1.f);
    }
    for (int k = threadIdx.x; k < j2; k += blockDim.x) {
        const long e = (long)slot * j2 + k, q = (long)slot * j + (k >> 1);
        const float x = a.x[e];
        if (away) { a.out[e] = x; continue; }
        const int sj = a.seen_j[q];
        if (!(a.maxvals[q] >= a.gate_min_score)) { a.out[e] = sj ? a.xhat[e] : x; continue; }
        const float T = a.gap[q] + dt;
        if (sj == 0 || !(T > 0.f) || !isfinite(T)) { a.xhat[e] = x; a.dxhat[e] = 0.f; a.out[e] = x; continue; }
        const float rd = (6.2831855f * a.d_cutoff) * T, ad = rd / (rd + 1.f);
        const float xh = a.xhat[e];
        const float dx = (x - xh) / T;
        const float dxh = ad * dx + (1.f - ad) * a.dxhat[e];
        const float speed = a.by_size ? fabsf(dxh) / size : fabsf(dxh);
        const float fc = a.min_cutoff + a.beta * speed;
        const float r = (6.2831855f * fc) * T, al = r / (r + 1.f);
        const float nx = al * x + (1.f - al) * xh;
        a.dxhat[e] = dxh; a.xhat[e] = nx; a.out[e] = nx;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < j; k += blockDim.x) {
        const long q = (long)slot * j + k;
        if (away) { a.seen_j[q] = 0; a.gap[q] = 0.f; continue; }
        if (!(a.maxvals[q] >= a.gate_min_score)) {
            if (dt > 0.f && isfinite(dt)) a.gap[q] += dt;
            continue;
        }
        a.seen_j[q] = 1; a.gap[q] = 0.f;
    }
}
