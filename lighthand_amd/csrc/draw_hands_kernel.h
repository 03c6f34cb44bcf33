// Device side of lh_draw_hands (draw_hands.hip): the skeleton overlay of the tracked top-down step -- ROI outline, bones and joint discs
// drawn into the frames in place, on the pixels around each hand only.  The rule is stated in include/lighthand_hip.h and restated in
// numpy by lighthand_amd/topdown.py (draw_hands_host); all arithmetic is fp32 in the order written (-ffp-contract=off), + - * /, sqrtf,
// floorf and comparisons only, so the host takes every texel bit for bit.
// (A mode of frames_crop_kernel<float>, as lh_tracks_manage's: the resource tables admit no new kernel symbol.  The launch is its own:
// DRAW_WGS workgroups per slot and dynamic LDS sized for this call's slots, so the crop's launches pay nothing.)
//
// Several slots on one frame composite in index order without a race and without atomics.  Every workgroup first works out the DRAW
// BOUNDS of all slots of its slot's frame -- the bounds of the slot's drawn primitives grown by r + 1 and clipped to the frame (outside
// them every coverage is 0, so they do not enter the rule) -- into LDS, and lists the slots that draw anything in ascending index.  A
// pixel is OWNED by the first slot of that list whose bounds contain it; the owner's workgroups walk the owner's bounds in a
// grid-stride loop, and the owning thread composites every listed slot whose bounds contain the pixel, in index order, then stores
// the texel once if any primitive covered it.  On 4:2:0 frames the unit is a 2 x 2 luma block with its chroma pair (the bounds are
// aligned to even pixels), so no texel has two writers either.
#pragma once
#include <type_traits>
#include "common.h"

#define DRAW_MAX 1024                                              // slots of one launch: 16-bit indices, 18 KB of LDS
#define DRAW_WGS 8                                                 // workgroups per slot, fixed: the grid does not depend on the data

// What lh_draw_hands passes beside CropArgs' own fields (dst / table / frame_stride: the frames; n_frames, hs, ws, format, pitch,
// dsc: their layout; src_frame, mat (may be null), h, w: the crop; n = b, j).
struct DrawArgs {
    const float *preds, *maxvals, *boxes, *palette;                // boxes may be null with by_size == 0
    const int *lost, *parents, *group;                             // lost may be null
    int n_groups, draw_roi;
    float min_score, line_radius, joint_radius, by_size, opacity;
};

__host__ __device__ inline size_t draw_lds_bytes(int b) { return (size_t)b * 16 + (size_t)(b + 1) / 2 * 4 + 4; }

// clamp((r + 0.5) - d, 0, 1), d the distance from (px, py) to the segment a -> a + (dx, dy); il2 = 1 / (dx*dx + dy*dy), read for l2 > 0 only
__device__ __forceinline__ float draw_cov(float px, float py, float ax, float ay, float dx, float dy, float l2, float il2, float r05) {
    const float qx = px - ax, qy = py - ay;
    float ex = qx, ey = qy;
    if (l2 > 0.f) {
        float t = (qx * dx + qy * dy) * il2;
        t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
        ex = qx - t * dx;
        ey = qy - t * dy;
    }
    const float v = r05 - sqrtf(ex * ex + ey * ey);
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

// the texel code of a blended value: floorf(c + 0.5) clamped to 0..top
__device__ __forceinline__ int draw_code(float c, float top) {
    const float v = floorf(c + 0.5f);
    return (int)(!(v >= 0.f) ? 0.f : (v > top ? top : v));
}

// The primitives of slot t in drawing order -- the four edges of the crop's quad, the bones, the joints -- as f(ax, ay, bx, by, r, row):
// a segment, its radius and its palette row.  A primitive with a coordinate or radius that is not finite, or a row outside the
// palette, is skipped; a lost slot draws its outline alone.
template <typename P, typename F>
__device__ __forceinline__ void draw_prims(const P& p, int t, F&& f) {
    const DrawArgs& a = p.dr;
    const int j = p.j, rows = a.n_groups + 2;
    const bool lost = a.lost && a.lost[t] != 0;
    float s = 0.f;
    if (a.by_size != 0.f) {
        const float* box = a.boxes + t * 4;
        const float bw = box[2] - box[0], bh = box[3] - box[1];
        s = bw > bh ? bw : bh;
    }
    const float r_line = a.line_radius + a.by_size * s, r_joint = a.joint_radius + a.by_size * s;
    auto emit = [&](float ax, float ay, float bx, float by, float r, int row) {
        if (isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by) && isfinite(r) && (unsigned)row < (unsigned)rows) f(ax, ay, bx, by, r, row);
    };
    if (p.mat && a.draw_roi) {
        const float* m = p.mat + t * 6;
        const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
        const float u1 = (float)p.w - 0.5f, v1 = (float)p.h - 0.5f;
#pragma unroll 1
        for (int e = 0; e < 4; ++e) {                              // corners (-.5, -.5), (w-.5, -.5), (w-.5, h-.5), (-.5, h-.5), each to the next
            const float ua = (e == 1 || e == 2) ? u1 : -0.5f, va = e >= 2 ? v1 : -0.5f;
            const float ub = (e == 0 || e == 1) ? u1 : -0.5f, vb = (e == 1 || e == 2) ? v1 : -0.5f;
            emit((m0 * ua + m1 * va) + m2, (m3 * ua + m4 * va) + m5, (m0 * ub + m1 * vb) + m2, (m3 * ub + m4 * vb) + m5, r_line,
                 a.n_groups + (lost ? 1 : 0));
        }
    }
    if (lost) return;
    const float* pt = a.preds + (long)t * j * 2;
    const float* mv = a.maxvals + (long)t * j;
#pragma unroll 1
    for (int i = 0; i < j; ++i) {
        const int pi = a.parents[i];
        if (pi < 0 || pi >= j || !(mv[pi] >= a.min_score) || !(mv[i] >= a.min_score)) continue;
        emit(pt[pi * 2], pt[pi * 2 + 1], pt[i * 2], pt[i * 2 + 1], r_line, a.group[i]);
    }
#pragma unroll 1
    for (int i = 0; i < j; ++i) {
        if (!(mv[i] >= a.min_score)) continue;
        emit(pt[i * 2], pt[i * 2 + 1], pt[i * 2], pt[i * 2 + 1], r_joint, a.group[i]);
    }
}

struct draw_rect { int x0, y0, x1, y1; };                          // inclusive; x0 > x1: nothing

__device__ __forceinline__ bool draw_in(const draw_rect r, int x, int y) { return x >= r.x0 && x <= r.x1 && y >= r.y0 && y <= r.y1; }

// One unit of the walk at (x, y), owned by this thread: the pixel (FMT = LH_FRAMES_RGB) or the 2 x 2 luma block and its chroma pair
// (LH_FRAMES_420: 8-bit samples, LH_FRAMES_420W: 16-bit, blended as u16 >> 6 on the 10-bit scale and stored as code << 6, so a texel
// nothing covers keeps its low six bits: it is not written).  e0: the unit's owner in the list.
template <int FMT, typename P>
__device__ __forceinline__ void draw_unit(const P& p, unsigned char* base, const draw_rect* s_bnd, const unsigned short* s_list, int n, int e0,
                                          int x, int y) {
    const DrawArgs& a = p.dr;
    const float opacity = a.opacity, fx = (float)x, fy = (float)y;
    if constexpr (FMT == LH_FRAMES_RGB) {
        unsigned char* px = base + (y * p.ws + x) * 3;
        float c0 = px[0], c1 = px[1], c2 = px[2];
        bool hit = false;
        for (int e = e0; e < n; ++e) {
            const int t = s_list[e];
            if (!draw_in(s_bnd[t], x, y)) continue;
            draw_prims(p, t, [&](float ax, float ay, float bx, float by, float r, int row) {
                const float dx = bx - ax, dy = by - ay, l2 = dx * dx + dy * dy, il2 = 1.f / l2;
                const float al = opacity * draw_cov(fx, fy, ax, ay, dx, dy, l2, il2, r + 0.5f);
                if (al > 0.f) {
                    const float* col = a.palette + row * 3;
                    c0 = c0 + al * (col[0] - c0);
                    c1 = c1 + al * (col[1] - c1);
                    c2 = c2 + al * (col[2] - c2);
                    hit = true;
                }
            });
        }
        if (hit) {
            px[0] = (unsigned char)draw_code(c0, 255.f);
            px[1] = (unsigned char)draw_code(c1, 255.f);
            px[2] = (unsigned char)draw_code(c2, 255.f);
        }
    } else {
        typedef typename std::conditional<FMT == LH_FRAMES_420W, unsigned short, unsigned char>::type U;
        constexpr int SB = sizeof(U), SHIFT = SB == 2 ? 6 : 0;
        constexpr float TOP = SB == 2 ? 1023.f : 255.f;
        const int o00 = y * p.pitch + x * SB, o10 = o00 + p.pitch;
        const int oc = (y >> 1) * p.dsc[0] + (x >> 1) * p.dsc[3], ocb = p.dsc[1] + oc, ocr = p.dsc[2] + oc;
        auto at = [&](int off) -> U* { return reinterpret_cast<U*>(base + off); };
        float l0 = (float)(*at(o00) >> SHIFT), l1 = (float)(*at(o00 + SB) >> SHIFT);
        float l2_ = (float)(*at(o10) >> SHIFT), l3 = (float)(*at(o10 + SB) >> SHIFT);
        float cb = (float)(*at(ocb) >> SHIFT), cr = (float)(*at(ocr) >> SHIFT);
        int hit = 0;                                               // bits 0..3: the luma pixels, bit 4: the chroma pair
        for (int e = e0; e < n; ++e) {
            const int t = s_list[e];
            if (!draw_in(s_bnd[t], x, y)) continue;
            draw_prims(p, t, [&](float ax, float ay, float bx, float by, float r, int row) {
                const float dx = bx - ax, dy = by - ay, l2 = dx * dx + dy * dy, il2 = 1.f / l2, r05 = r + 0.5f;
                const float k0 = draw_cov(fx, fy, ax, ay, dx, dy, l2, il2, r05), k1 = draw_cov(fx + 1.f, fy, ax, ay, dx, dy, l2, il2, r05);
                const float k2 = draw_cov(fx, fy + 1.f, ax, ay, dx, dy, l2, il2, r05), k3 = draw_cov(fx + 1.f, fy + 1.f, ax, ay, dx, dy, l2, il2, r05);
                const float* col = a.palette + row * 3;
                const float cy_ = col[0];
                const float a0 = opacity * k0, a1 = opacity * k1, a2 = opacity * k2, a3 = opacity * k3;
                if (a0 > 0.f) { l0 = l0 + a0 * (cy_ - l0); hit |= 1; }
                if (a1 > 0.f) { l1 = l1 + a1 * (cy_ - l1); hit |= 2; }
                if (a2 > 0.f) { l2_ = l2_ + a2 * (cy_ - l2_); hit |= 4; }
                if (a3 > 0.f) { l3 = l3 + a3 * (cy_ - l3); hit |= 8; }
                const float ac = (opacity * ((k0 + k1) + (k2 + k3))) * 0.25f;
                if (ac > 0.f) {
                    cb = cb + ac * (col[1] - cb);
                    cr = cr + ac * (col[2] - cr);
                    hit |= 16;
                }
            });
        }
        if (hit & 1) *at(o00) = (U)(draw_code(l0, TOP) << SHIFT);
        if (hit & 2) *at(o00 + SB) = (U)(draw_code(l1, TOP) << SHIFT);
        if (hit & 4) *at(o10) = (U)(draw_code(l2_, TOP) << SHIFT);
        if (hit & 8) *at(o10 + SB) = (U)(draw_code(l3, TOP) << SHIFT);
        if (hit & 16) {
            *at(ocb) = (U)(draw_code(cb, TOP) << SHIFT);
            *at(ocr) = (U)(draw_code(cr, TOP) << SHIFT);
        }
    }
}

// The owner's walk over its draw bounds: workgroup `part` of DRAW_WGS, one unit per thread and step.
template <int FMT, typename P>
__device__ __forceinline__ void draw_walk(const P& p, unsigned char* base, const draw_rect* s_bnd, const unsigned short* s_list, int n, int slot,
                                          int part) {
    constexpr int SH = FMT == LH_FRAMES_RGB ? 0 : 1;
    const draw_rect own = s_bnd[slot];
    const int nx = (own.x1 - own.x0 + 1) >> SH, ny = (own.y1 - own.y0 + 1) >> SH;
    for (int q = part * blockDim.x + threadIdx.x; q < nx * ny; q += DRAW_WGS * blockDim.x) {
        const int uy = q / nx, ux = q - uy * nx;
        const int x = own.x0 + (ux << SH), y = own.y0 + (uy << SH);
        int e0 = 0;
        while (e0 < n && !draw_in(s_bnd[s_list[e0]], x, y)) ++e0;  // the unit's owner: the first listed slot that contains it
        if (e0 >= n || s_list[e0] != slot) continue;
        draw_unit<FMT>(p, base, s_bnd, s_list, n, e0, x, y);
    }
}

// grid (b * DRAW_WGS), 256 threads, dynamic LDS draw_lds_bytes(b): lh_draw_hands' launch alone
template <typename P>
__device__ __forceinline__ void draw_hands_slot(const P& p, unsigned char* lds) {
    const int b = p.n, slot = blockIdx.x / DRAW_WGS, part = blockIdx.x - slot * DRAW_WGS;
    const int f = p.src_frame[slot];
    if (f < 0 || f >= p.n_frames) return;                          // an empty slot draws nothing: never an address
    unsigned char* base;
    if (p.table) {
        const long long at = p.table[f];                           // a scalar load; tested before it becomes an address
        if (at == 0) return;                                       // an unbound surface: skipped
        base = reinterpret_cast<unsigned char*>(at);
    } else {
        base = (unsigned char*)p.dst + (long)f * p.frame_stride;
    }
    draw_rect* s_bnd = reinterpret_cast<draw_rect*>(lds);
    unsigned short* s_list = reinterpret_cast<unsigned short*>(s_bnd + b);
    int* s_n = reinterpret_cast<int*>(lds + (size_t)b * 16 + (size_t)(b + 1) / 2 * 4);
    const bool even = p.format != LH_FRAMES_RGB;
    const float wl = (float)(p.ws - 1), hl = (float)(p.hs - 1);
    for (int t = threadIdx.x; t < b; t += blockDim.x) {
        draw_rect bd = {1, 1, 0, 0};
        if (p.src_frame[t] == f) {
            float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
            draw_prims(p, t, [&](float ax, float ay, float bx, float by, float r, int) {
                const float g = r + 1.f;
                lo_x = fminf(lo_x, fminf(ax, bx) - g); hi_x = fmaxf(hi_x, fmaxf(ax, bx) + g);
                lo_y = fminf(lo_y, fminf(ay, by) - g); hi_y = fmaxf(hi_y, fmaxf(ay, by) + g);
            });
            if (lo_x <= wl && hi_x >= 0.f && lo_y <= hl && hi_y >= 0.f) {          // false without a primitive
                bd.x0 = (int)fmaxf(floorf(lo_x), 0.f); bd.x1 = (int)fminf(ceilf(hi_x), wl);
                bd.y0 = (int)fmaxf(floorf(lo_y), 0.f); bd.y1 = (int)fminf(ceilf(hi_y), hl);
                if (even) { bd.x0 &= ~1; bd.y0 &= ~1; bd.x1 |= 1; bd.y1 |= 1; }    // whole 2 x 2 blocks (hs and ws are even)
            }
        }
        s_bnd[t] = bd;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int t = 0; t < b; ++t)
            if (s_bnd[t].x0 <= s_bnd[t].x1) s_list[n++] = (unsigned short)t;
        *s_n = n;
    }
    __syncthreads();
    const int n = *s_n;
    if (s_bnd[slot].x0 > s_bnd[slot].x1) return;
    if (p.format == LH_FRAMES_RGB) draw_walk<LH_FRAMES_RGB>(p, base, s_bnd, s_list, n, slot, part);
    else if (p.format == LH_FRAMES_420) draw_walk<LH_FRAMES_420>(p, base, s_bnd, s_list, n, slot, part);
    else draw_walk<LH_FRAMES_420W>(p, base, s_bnd, s_list, n, slot, part);
}
