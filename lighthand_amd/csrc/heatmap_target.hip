// Heat-map targets: the Gaussian renderers (quantised, visibility-weighted, sub-pixel) and the alternate GenerateHeatmap renderer.
#include "common.h"

// generate_target (src/tools/dataset.py:171-186).  WEIGHTED renders upstream's target_weight with it (`if v > 0.5:`): weight =
// visibility x "some part of the patch lies inside the map", a joint of weight 0 gets a zero map, and the thread that owns pixel
// (0, 0) of a plane writes that plane's weight.  A compile-time switch: the unweighted instantiation never reads vis / weight
// (passed as null).
// SUB (lh_gaussian_target_sub, DARK's unbiased encoding): the same window, skip test and weight, but the value inside the window
// is the Gaussian around the joint's real-valued heat-map position, one expf per pixel; `patch` is not read.  A second
// compile-time switch, so the two quantised instantiations keep their code.
template <bool WEIGHTED, bool SUB = false>
__global__ void gaussian_target_kernel(const float* joints, int jstride, const float* vis, int vstride, const float* patch,
                                       int radius, float* target, float* weight, int bj, int size, float sigma) {
    const long total = (long)bj * size * size;
    const int pw = 2 * radius + 1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % size);
        const long t = i / size;
        const int y = (int)(t % size);
        const long j = t / size;
        const float jx = joints[j * jstride], jy = joints[j * jstride + 1];
        // int(v / 4 + 0.5): truncation toward zero, like Python's int()
        const int mx = (int)(jx * 0.25f + 0.5f), my = (int)(jy * 0.25f + 0.5f);
        const int x0 = mx - radius, y0 = my - radius, x1 = mx + radius + 1, y1 = my + radius + 1;
        const bool skip = x0 >= size || y0 >= size || x1 < 0 || y1 < 0;
        bool draw = !skip;
        float w = 0.f;
        if constexpr (WEIGHTED) {
            const float v = vis ? vis[j * vstride] : 1.f;
            w = (v > 0.5f ? v : 0.f) * (skip ? 0.f : 1.f);
            draw = w > 0.f;
        }
        float out = 0.f;
        if (draw && x >= x0 && x < x1 && y >= y0 && y < y1) {
            if constexpr (SUB) {
                const float dx = (float)x - jx * 0.25f, dy = (float)y - jy * 0.25f;
                out = expf(-(dx * dx + dy * dy) / (2.f * sigma * sigma));
            } else {
                out = patch[(y - y0) * pw + (x - x0)];
            }
        }
        target[i] = out;
        if constexpr (WEIGHTED)
            if (x == 0 && y == 0) weight[j] = w;
    }
}

// GenerateHeatmap (src/utils/dataset_loader.py:22-53), the alternate renderer: points are ALREADY in heat-map coordinates,
// sigma = res / 64 (an integer here), patch of (6 * sigma + 3)^2 centred on int(point), np.maximum blend with the zero
// map (= plain placement: every joint owns its plane); a joint is skipped when x <= 0 or int(point) lies outside the map.
__global__ void gaussian_target_alt_kernel(const float* points, int pstride, const float* patch, int sigma, float* target,
                                           int bj, int res) {
    const long total = (long)bj * res * res;
    const int pw = 6 * sigma + 3;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % res);
        const long t = i / res;
        const int y = (int)(t % res);
        const long j = t / res;
        const float fx = points[j * pstride], fy = points[j * pstride + 1];
        float v = 0.f;
        if (fx > 0.f) {
            const int px = (int)fx, py = (int)fy;                    // Python int(): truncation toward zero
            if (px >= 0 && py >= 0 && px < res && py < res) {
                const int ulx = px - 3 * sigma - 1, uly = py - 3 * sigma - 1;
                const int gx = x - ulx, gy = y - uly;                // hms[aa:bb, cc:dd] <- g[a:b, c:d]: same offset on both axes
                if (gx >= 0 && gx < pw && gy >= 0 && gy < pw) v = patch[gy * pw + gx];
            }
        }
        target[i] = v;
    }
}

extern "C" int lh_gaussian_target_alt(const float* points, int pstride, const float* patch, int sigma, float* target,
                                      int b, int j, int res, void* stream) {
    LH_REQUIRE(points && patch && target && pstride >= 2 && b > 0 && j > 0 && res > 0 && sigma >= 1 && res == 64 * sigma,
               "lh_gaussian_target_alt: bad arguments (res must be 64 * sigma, sigma a positive integer)");
    const long total = (long)b * j * res * res;
    const int grid = lh_grid(total, 4096);
    hipLaunchKernelGGL(gaussian_target_alt_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, points, pstride, patch, sigma,
                       target, b * j, res);
    LH_LAUNCH_CHECK("gaussian_target_alt launch");
    return LH_OK;
}

extern "C" int lh_gaussian_target(const float* joints, int jstride, const float* patch, int radius, float* target,
                                  int b, int j, int size, void* stream) {
    LH_REQUIRE(joints && patch && target && jstride >= 2 && b > 0 && j > 0 && size > 0 && radius >= 0,
               "lh_gaussian_target: bad arguments");
    hipLaunchKernelGGL(gaussian_target_kernel<false>, dim3(lh_grid((long)b * j * size * size, 4096)), dim3(256), 0, (hipStream_t)stream,
                       joints, jstride, (const float*)nullptr, 0, patch, radius, target, (float*)nullptr, b * j, size, 0.f);
    LH_LAUNCH_CHECK("gaussian_target launch");
    return LH_OK;
}

extern "C" int lh_gaussian_target_w(const float* joints, int jstride, const float* vis, int vstride, const float* patch, int radius,
                                    float* target, float* weight, int b, int j, int size, void* stream) {
    LH_REQUIRE(joints && patch && target && weight && jstride >= 2 && (!vis || vstride >= 1) && b > 0 && j > 0 && size > 0 && radius >= 0,
               "lh_gaussian_target_w: bad arguments");
    hipLaunchKernelGGL(gaussian_target_kernel<true>, dim3(lh_grid((long)b * j * size * size, 4096)), dim3(256), 0, (hipStream_t)stream,
                       joints, jstride, vis, vstride, patch, radius, target, weight, b * j, size, 0.f);
    LH_LAUNCH_CHECK("gaussian_target_w launch");
    return LH_OK;
}

extern "C" int lh_gaussian_target_sub(const float* joints, int jstride, const float* vis, int vstride, int radius, float sigma,
                                      float* target, float* weight, int b, int j, int size, void* stream) {
    LH_REQUIRE(joints && target && jstride >= 2 && (!vis || vstride >= 1) && b > 0 && j > 0 && size > 0 && radius >= 0 && sigma > 0.f,
               "lh_gaussian_target_sub: bad arguments (sigma must be positive)");
    const dim3 grid(lh_grid((long)b * j * size * size, 4096));
    if (weight)
        hipLaunchKernelGGL((gaussian_target_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, joints, jstride, vis, vstride,
                           (const float*)nullptr, radius, target, weight, b * j, size, sigma);
    else
        hipLaunchKernelGGL((gaussian_target_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, joints, jstride,
                           (const float*)nullptr, 0, (const float*)nullptr, radius, target, (float*)nullptr, b * j, size, sigma);
    LH_LAUNCH_CHECK("gaussian_target_sub launch");
    return LH_OK;
}
