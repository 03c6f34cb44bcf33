// Instantiations of the LDS-DMA weight-gradient kernel (wgrad_ring_kernel.h) for one element type: every compiled-in configuration of
// wgrad_cfgs.h in the single-problem and table forms -- the 8-wave 256 x 256 tile included (the late stages' and the head's gradients
// are the ones that run split-free in a shared grid) -- and the 4-wave tiles in the multi-problem form (the batched layers are the
// small ones).  A unit includes this and expands LH_WGRAD_RING_LAUNCHERS or LH_WGRAD_TABLE_LAUNCHER once.
#pragma once
#include "wgrad_plan.h"

// Raise the kernel's dynamic LDS limit when its ring needs more than the default 64 KiB, then launch `grid` workgroups.
template <int BO, int BI, int WO, int WI, int D, int KPS, typename... P, typename... A>
static int launch_wgrad_ring(void (*kernel)(P...), const char* what, int grid, hipStream_t s, const A&... args) {
    constexpr int lds = D * KPS * (BO * 2 + BI * 2);
    static_assert(lds <= 160 * 1024, "LDS budget");
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) {
            lh_set_error("%s: cannot raise dynamic LDS to %d bytes: %s", what, lds, hipGetErrorString(e));
            return LH_ERR_HIP;
        }
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * WO * WI), lds, s, args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        lh_set_error("%s launch: %s", what, hipGetErrorString(e));
        return LH_ERR_HIP;
    }
    return LH_OK;
}

// multi-problem form: the 4-wave tiles only; 1 (not compiled in) for anything else
template <typename T, int BO, int BI, int WO, int WI, int D, int KPS>
static int launch_wgrad_ring_multi(const LhMulti<WgradArgs>& m, hipStream_t s) {
    if constexpr (WO * WI != 4) return 1;
    else return launch_wgrad_ring<BO, BI, WO, WI, D, KPS>(&wgrad_ring_multi_kernel<T, BO, BI, WO, WI, D, KPS>, "wgrad_ring_multi", m.first[m.n], s, m);
}

// One `if` per configuration of wgrad_cfgs.h; `elem` is the launcher's element type.  The launchers return 1 when none matches.
#define LH_WGRAD_RING_CASE(BO, BI, WO, WI, D, KPS)                \
    if (c.bo == BO && c.bi == BI && c.depth == D && c.kps == KPS) \
        return launch_wgrad_ring<BO, BI, WO, WI, D, KPS>(&wgrad_ring_kernel<elem, BO, BI, WO, WI, D, KPS>, "wgrad_ring", a.tiles * a.ntaps * a.nsplit, s, a);
#define LH_WGRAD_MULTI_CASE(BO, BI, WO, WI, D, KPS) \
    if (c.bo == BO && c.bi == BI && c.depth == D && c.kps == KPS) return launch_wgrad_ring_multi<elem, BO, BI, WO, WI, D, KPS>(m, s);
#define LH_WGRAD_TABLE_CASE(BO, BI, WO, WI, D, KPS)       \
    if (bo == BO && bi == BI && depth == D && kps == KPS) \
        return launch_wgrad_ring<BO, BI, WO, WI, D, KPS>(&wgrad_ring_table_kernel<elem, BO, BI, WO, WI, D, KPS>, "wgrad_ring_table", n_items, s, tab, items);

#define LH_WGRAD_RING_LAUNCHERS(SINGLE, MULTI, T)                                    \
    int SINGLE(const WgradArgs& a, const WgradPlan& c, hipStream_t s) {              \
        typedef T elem;                                                              \
        LH_WGRAD_CFGS(LH_WGRAD_RING_CASE)                                            \
        return 1;                                                                    \
    }                                                                                \
    int MULTI(const LhMulti<WgradArgs>& m, const WgradPlan& c, hipStream_t s) {      \
        typedef T elem;                                                              \
        LH_WGRAD_CFGS(LH_WGRAD_MULTI_CASE)                                           \
        return 1;                                                                    \
    }
#define LH_WGRAD_TABLE_LAUNCHER(NAME, T)                                                                                \
    int NAME(const WgradArgs* tab, const int2* items, int n_items, int bo, int bi, int kps, int depth, hipStream_t s) { \
        typedef T elem;                                                                                                 \
        LH_WGRAD_CFGS(LH_WGRAD_TABLE_CASE)                                                                              \
        return 1;                                                                                                       \
    }
