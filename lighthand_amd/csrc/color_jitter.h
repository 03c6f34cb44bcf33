// torchvision's ColorJitter on one pixel, shared by the uint8 input kernels (ingest.hip) and the frame crop (frames_crop_kernel.h).
// The random draw stays on the host (ColorJitter.get_params): per image four factors (brightness, contrast,
// saturation, hue) and the op order (four op ids 0..3, negative = skip) arrive as device arrays.  Contrast blends
// with the mean grey level of the WHOLE image as it is when the op runs, so a first pass reduces that mean (of the
// image after the ops that precede contrast) into fp64 partial sums, and a second pass applies everything.
#pragma once

__device__ __forceinline__ float cj_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float cj_gray(const float* c) { return 0.2989f * c[0] + 0.587f * c[1] + 0.114f * c[2]; }
__device__ __forceinline__ void cj_blend(float* c, float o0, float o1, float o2, float r) {
    c[0] = cj_clamp01(r * c[0] + (1.f - r) * o0);
    c[1] = cj_clamp01(r * c[1] + (1.f - r) * o1);
    c[2] = cj_clamp01(r * c[2] + (1.f - r) * o2);
}
__device__ __forceinline__ void cj_hue(float* c, float f) {
    const float r = c[0], g = c[1], b = c[2];
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eq ? 1.f : maxc);
    const float div = eq ? 1.f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    float h = 0.f;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = 2.f + rc - bc;
    else h = 4.f + gc - rc;
    h = fmodf(h / 6.f + 1.f, 1.f);
    h = fmodf(h + f, 1.f);
    if (h < 0.f) h += 1.f;
    const float h6 = h * 6.f;
    const float fl = floorf(h6);
    const float fr = h6 - fl;
    int i = (int)fl % 6;
    if (i < 0) i += 6;
    const float v = maxc;
    const float p = cj_clamp01(v * (1.f - s)), q = cj_clamp01(v * (1.f - s * fr)), t = cj_clamp01(v * (1.f - s * (1.f - fr)));
    switch (i) {
        case 0: c[0] = v; c[1] = t; c[2] = p; break;
        case 1: c[0] = q; c[1] = v; c[2] = p; break;
        case 2: c[0] = p; c[1] = v; c[2] = t; break;
        case 3: c[0] = p; c[1] = q; c[2] = v; break;
        case 4: c[0] = t; c[1] = p; c[2] = v; break;
        default: c[0] = v; c[1] = p; c[2] = q; break;
    }
}
// ops order[first .. last) on one pixel; `mean` = the image's grey mean for the contrast op
__device__ __forceinline__ void cj_apply(float* c, const float* f, const int* order, int first, int last, float mean) {
    for (int k = first; k < last; ++k) {
        const int op = order[k];
        if (op == 0) cj_blend(c, 0.f, 0.f, 0.f, f[0]);
        else if (op == 1) cj_blend(c, mean, mean, mean, f[1]);
        else if (op == 2) { const float g = cj_gray(c); cj_blend(c, g, g, g, f[2]); }
        else if (op == 3) cj_hue(c, f[3]);
    }
}

constexpr int CJ_STRIPS = 32;                             // fp64 partial sums of the grey mean per image (or crop slot)
