// Validation metrics on decoded keypoints: per-sample PCK / EPE counts and the PCK curve over a list of thresholds.
#include "common.h"

// PCK_2d_loss(T, 'proportion') + EPE_train on the device (src/utils/loss.py:50-67,116-148): one wave per
// sample.  wrong[b] = #joints whose error / bbox-diagonal(gt) > T; epe[b] = sum of errors of joints 1..J-2 (the
// reference's joint range quirk).  Sums over the batch are left to the caller (device tensors, no host sync).
__global__ __launch_bounds__(64) void keypoint_metrics_kernel(const float* pred, const float* gt, int gt_stride, int j, float T,
                                                              int* wrong, float* epe) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* g = gt + (long)b * j * gt_stride;
    const float* p = pred + (long)b * j * 2;
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int k = lane; k < j; k += 64) {
        const float x = g[k * gt_stride], y = g[k * gt_stride + 1];
        xmin = fminf(xmin, x); xmax = fmaxf(xmax, x); ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        xmin = fminf(xmin, __shfl_xor(xmin, o)); xmax = fmaxf(xmax, __shfl_xor(xmax, o));
        ymin = fminf(ymin, __shfl_xor(ymin, o)); ymax = fmaxf(ymax, __shfl_xor(ymax, o));
    }
    const float diag = sqrtf((xmax - xmin) * (xmax - xmin) + (ymax - ymin) * (ymax - ymin));
    int w = 0;
    float e = 0.f;
    for (int k = lane; k < j; k += 64) {
        const float dx = g[k * gt_stride] - p[k * 2], dy = g[k * gt_stride + 1] - p[k * 2 + 1];
        const float dist = sqrtf(dx * dx + dy * dy);
        if (dist / diag > T) ++w;
        if (k >= 1 && k <= j - 2) e += dist;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { w += __shfl_xor(w, o); e += __shfl_xor(e, o); }
    if (lane == 0) { wrong[b] = w; epe[b] = e; }
}

extern "C" int lh_keypoint_metrics(const float* pred, const float* gt, int gt_stride, int b, int j, float T, int* wrong,
                                   float* epe, void* stream) {
    LH_REQUIRE(pred && gt && wrong && epe && b > 0 && j > 2 && gt_stride >= 2, "lh_keypoint_metrics: bad arguments");
    hipLaunchKernelGGL(keypoint_metrics_kernel, dim3(b), dim3(64), 0, (hipStream_t)stream, pred, gt, gt_stride, j, T, wrong, epe);
    LH_LAUNCH_CHECK("keypoint_metrics launch");
    return LH_OK;
}

// PCK curve / AUC: pred_eval (src/utils/argparser.py:326-388) on the device: for every threshold, the number of
// VISIBLE joints (gt[..][2] == 1) whose error -- pixel distance, divided by the sample's bbox size when bb is given ('pckb') --
// is < thr[t].  float64 like the NumPy original, integer atomics (exact, order independent: ranks add their counts with one
// small all-reduce).  diff_row[s] = sum of the pixel errors of ALL joints of sample s (the EPE numerator).
__global__ void pck_curve_kernel(const float* pred, const float* gt, int gt_stride, const float* bb, int n, int j,
                                 const double* thr, int nthr, unsigned long long* counts, unsigned long long* nvis,
                                 double* diff_row) {
    const int sidx = blockIdx.x;
    if (sidx >= n) return;
    __shared__ double err[64];
    __shared__ int vis[64];
    for (int k = threadIdx.x; k < j; k += blockDim.x) {
        const float* g = gt + ((long)sidx * j + k) * gt_stride;
        const float* q = pred + ((long)sidx * j + k) * 2;
        const double dx = (double)g[0] - (double)q[0], dy = (double)g[1] - (double)q[1];
        err[k] = sqrt(dx * dx + dy * dy);
        vis[k] = g[2] == 1.f ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        int nv = 0;
        for (int k = 0; k < j; ++k) { sum += err[k]; nv += vis[k]; }
        diff_row[sidx] = sum;
        if (nv) atomicAdd(nvis, (unsigned long long)nv);
    }
    const double scale = bb ? (double)bb[sidx] : 1.0;
    for (int t = threadIdx.x; t < nthr; t += blockDim.x) {
        int c = 0;
        for (int k = 0; k < j; ++k)
            if (vis[k] && err[k] / scale < thr[t]) ++c;
        if (c) atomicAdd(counts + t, (unsigned long long)c);
    }
}

extern "C" int lh_pck_curve(const float* pred, const float* gt, int gt_stride, const float* bb, int n, int j, const double* thr,
                            int nthr, unsigned long long* counts, unsigned long long* nvis, double* diff_row, void* stream) {
    LH_REQUIRE(pred && gt && thr && counts && nvis && diff_row && n > 0 && j > 0 && j <= 64 && gt_stride >= 3 && nthr > 0,
               "lh_pck_curve: bad arguments (j <= 64, gt rows of >= 3 values: x, y, visibility)");
    hipLaunchKernelGGL(pck_curve_kernel, dim3(n), dim3(128), 0, (hipStream_t)stream, pred, gt, gt_stride, bb, n, j, thr, nthr,
                       counts, nvis, diff_row);
    LH_LAUNCH_CHECK("pck_curve launch");
    return LH_OK;
}
