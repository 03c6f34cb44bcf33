// Multi-problem launches: up to LH_MULTI_MAX independent problems of ONE kernel instantiation run as ONE grid.
// The per-problem argument blocks travel BY VALUE in the kernel-argument segment (an array indexed with a wave-uniform
// index: scalar loads, no table in device memory, nothing to upload, capturable like any other launch); workgroup b
// belongs to problem i with first[i] <= b < first[i + 1] and runs that problem's body with its local block index.
// Used for the parallel branches of HRNet (pose_hrnet.py:139-185, 247-265: the same layer position of 2-4 branches),
// whose kernels are a few microseconds of work each: one launch instead of four.
#pragma once
#include "common.h"

constexpr int LH_MULTI_MAX = 4;

template <typename A> struct LhMulti {
    A a[LH_MULTI_MAX];
    int first[LH_MULTI_MAX + 1];
    int n;
};

// problem index of this workgroup; bid / nblk = its block index and block count inside that problem
template <typename M> __device__ __forceinline__ int lh_multi_pick(const M& m, int& bid, int& nblk) {
    const int b = blockIdx.x;
    int i = 0;
    while (i + 1 < m.n && b >= m.first[i + 1]) ++i;
    bid = b - m.first[i];
    nblk = m.first[i + 1] - m.first[i];
    return i;
}

// One problem or several through ONE pair of kernels.  A pass is a struct `Body` with `using Args = ...` (its by-value
// argument block) and `static __device__ void run(const Args&, int bid, int nblk)`, written against the block index and
// block count it is given: lh_one_kernel hands it the grid's, lh_multi_kernel those of the problem the workgroup
// belongs to.  (256 threads: what every elementwise BatchNorm / ReLU pass is written for.)
template <class Body> __global__ __launch_bounds__(256) void lh_one_kernel(const typename Body::Args p) {
    Body::run(p, blockIdx.x, gridDim.x);
}
template <class Body> __global__ __launch_bounds__(256) void lh_multi_kernel(const LhMulti<typename Body::Args> m) {
    int bid, nblk;
    const int i = lh_multi_pick(m, bid, nblk);
    Body::run(m.a[i], bid, nblk);
}

// n == 1: a plain launch with grid[0] workgroups; 1 < n <= LH_MULTI_MAX: one launch over the concatenated grids
template <class Body> void lh_launch(const typename Body::Args* const* a, const int* grid, int n, hipStream_t s) {
    if (n == 1) {
        hipLaunchKernelGGL((lh_one_kernel<Body>), dim3(grid[0]), dim3(256), 0, s, *a[0]);
        return;
    }
    LhMulti<typename Body::Args> m;
    m.n = n; m.first[0] = 0;
    for (int i = 0; i < n; ++i) { m.a[i] = *a[i]; m.first[i + 1] = m.first[i] + grid[i]; }
    hipLaunchKernelGGL((lh_multi_kernel<Body>), dim3(m.first[n]), dim3(256), 0, s, m);
}

// the same for n launch records (a struct with `grid` and the argument block `args` of this pass among its members)
template <class Body, class Rec>
void lh_launch_records(const Rec* const* L, int n, const typename Body::Args Rec::*args, hipStream_t s) {
    const typename Body::Args* a[LH_MULTI_MAX];
    int grid[LH_MULTI_MAX];
    for (int i = 0; i < n; ++i) { a[i] = &(L[i]->*args); grid[i] = L[i]->grid; }
    lh_launch<Body>(a, grid, n, s);
}
