// Weight gradient, C entry points: plan queries, the single-problem launches (LDS-DMA ring kernel, wgrad_ring_kernel.h, or the
// register-staged kernel, wgrad_kernel.h), the fold of the pixel-split slabs (wgrad_reduce.h) and the four-at-a-time form.
// The planner is wgrad_plan.h; the table form is wgrad_table.hip.
#include "wgrad_plan.h"
#include "wgrad_kernel.h"
#include "wgrad_reduce.h"
#include <algorithm>
#include <mutex>

__global__ __launch_bounds__(256) void wgrad_reduce_contig_kernel(const WreduceArgs p) {
    extern __shared__ float tile[];                       // [256][ntaps + 1]
    wgrad_reduce_contig_body(p, tile, blockIdx.x);
}
__global__ void wgrad_reduce_kernel(const WreduceArgs p) { wgrad_reduce_body(p, blockIdx.x, gridDim.x); }
__global__ void wgrad_reduce_multi_kernel(const LhMulti<WreduceArgs> m) {
    int bid, nblk;
    const int i = lh_multi_pick(m, bid, nblk);
    wgrad_reduce_body(m.a[i], bid, nblk);
}

extern "C" int lh_wgrad_tile(const lh_igemm_desc* d, int n_out, int n_in, int dtype, int* bo, int* bi, int* nsplit, int* ring) {
    LH_REQUIRE(d && bo && bi && nsplit && ring, "lh_wgrad_tile: null pointer");
    WgradPlan c;
    const int rc = wgrad_plan(d, n_out, n_in, dtype, &c);
    if (rc) return rc;
    *bo = c.bo; *bi = c.bi; *nsplit = c.nsplit;
    *ring = c.kps ? c.kps * 10 + c.depth : 0;           // pixel rows per stage * 10 + ring depth; 0 = register-staged kernel
    return LH_OK;
}

// Candidate plans of the LDS-DMA kernel for this launch: every compiled-in (tile, stage, depth) that fits, each with the
// split counts that aim at 256 .. 2048 workgroups.  out: 5 ints per candidate = bo, bi, cfg[7] encoding, workgroups, slab MiB.
extern "C" int lh_wgrad_candidates(const lh_igemm_desc* d, int n_out, int n_in, int dtype, int* out, int max) {
    if (!d || !out || max <= 0 || !wgrad_ring_ok(d, lh_dtype_size(dtype))) return 0;
    int k = 0;
    for (int i = 0; i < kNWCfg; ++i) {
        const WgradCfg& c = kWCfg[i];
        if (!wcfg_fits(c, n_out, n_in)) continue;
        const long tiles = (long)((n_out + c.bo - 1) / c.bo) * ((n_in + c.bi - 1) / c.bi) * d->ntaps;
        const long stages = ((long)d->n * d->ho * d->wo + c.kps - 1) / c.kps;
        int seen[12], nseen = 0;
        const long targets[5] = {256, 512, 1024, 2048, 4096};
        const bool big = c.bo * c.bi >= 256 * 256;
        for (int t = 0; t < (big ? 8 : 11) && k < max; ++t) {
            int ns, sps;
            if (t < 5) {
                wgrad_splits(d, n_out, n_in, c.bo, c.bi, c.kps, targets[t], &ns, &sps);
            } else {
                // also offer the split counts that fill the 256 CUs exactly once, twice, ... (the 8-wave tile runs one workgroup
                // per CU: 1 - 3 rounds; the 4-wave tiles two to four per CU: 1 - 6 x 256 workgroups): the targets above round the
                // split count UP, and a launch of 576 workgroups on 512 slots runs a second round for its last 64
                const long fill = 256L * (t - 4) / tiles;
                if (fill < 1 || fill > 0xffff) continue;
                sps = (int)((stages + fill - 1) / fill);
                ns = (int)((stages + sps - 1) / sps);
                if (sps * c.kps < 256) continue;
            }
            bool dup = ns > 0xffff;
            for (int q = 0; q < nseen; ++q) dup = dup || seen[q] == ns;
            if (dup) continue;
            seen[nseen++] = ns;
            out[5 * k] = c.bo; out[5 * k + 1] = c.bi; out[5 * k + 2] = ns | (c.kps << 16) | (c.depth << 24);
            out[5 * k + 3] = (int)(tiles * ns);
            out[5 * k + 4] = (int)(((long)ns * d->ntaps * n_out * n_in * 4) >> 20);
            ++k;
        }
    }
    return k;
}

extern "C" size_t lh_wgrad_slab_bytes(const lh_igemm_desc* d, int n_out, int n_in, int dtype) {
    WgradPlan c;
    if (wgrad_plan(d, n_out, n_in, dtype, &c)) return 0;
    return (size_t)c.nsplit * d->ntaps * n_out * n_in * sizeof(float);
}

extern "C" size_t lh_wgrad_workspace_bytes(const lh_igemm_desc* d, int n_out, int n_in, int dtype) {
    return lh_wgrad_slab_bytes(d, n_out, n_in, dtype);
}

// 16 zero bytes in device memory (one copy per device), the source of every masked LDS-DMA lane.
__device__ __attribute__((aligned(16))) unsigned int lh_wzero_page[4] = {0u, 0u, 0u, 0u};

const unsigned char* wgrad_zero_page() {
    static std::mutex mu;
    static const unsigned char* ptr[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!ptr[dev]) {
        void* q = nullptr;
        if (hipGetSymbolAddress(&q, HIP_SYMBOL(lh_wzero_page)) != hipSuccess) return nullptr;
        ptr[dev] = (const unsigned char*)q;
    }
    return ptr[dev];
}

template <typename T, int BO, int BI, int WO, int WI>
static int launch_wgrad(const WgradArgs& a, hipStream_t s) {
    constexpr int ES = sizeof(T);
    constexpr int lds = 2 * WFrag<T>::KP * (BO * ES + BI * ES + 2 * WFrag<T>::PAD);
    dim3 grid(ceil_div(a.n_out, BO) * a.i_tiles, a.ntaps, a.nsplit);
    hipLaunchKernelGGL((wgrad_kernel<T, BO, BI, WO, WI>), grid, dim3(256), lds, s, a);
    LH_LAUNCH_CHECK("wgrad launch");
    return LH_OK;
}

// Launch one filled argument block under its plan: the LDS-DMA ring kernel (16-bit types, 16-byte aligned pixel rows), which reads
// its masked lanes from the zero page, or the register-staged kernel.
static int wgrad_launch(WgradArgs& a, const WgradPlan& c, int dtype, hipStream_t s) {
    if (c.kps) {
        a.zero = wgrad_zero_page();
        LH_REQUIRE(a.zero, "lh_wgrad: cannot resolve the zero page on this device");
        const int r = dtype == LH_BF16 ? lh_wgrad_ring_launch_bf16(a, c, s) : lh_wgrad_ring_launch_f16(a, c, s);
        if (r == 1) {
            lh_set_error("lh_wgrad: no kernel for tile %dx%d stage %d depth %d", c.bo, c.bi, c.kps, c.depth);
            return LH_ERR_UNSUPPORTED;
        }
        return r;
    }
#define LH_WT(T)                                                                 \
    if (c.bo == 128 && c.bi == 128) return launch_wgrad<T, 128, 128, 2, 2>(a, s); \
    if (c.bo == 128 && c.bi == 64) return launch_wgrad<T, 128, 64, 4, 1>(a, s);   \
    if (c.bo == 64 && c.bi == 128) return launch_wgrad<T, 64, 128, 1, 4>(a, s);   \
    return launch_wgrad<T, 64, 64, 2, 2>(a, s);
    switch (dtype) {
        case LH_BF16: { LH_WT(bf16) }
        case LH_F16: { LH_WT(f16) }
        case LH_F32: { LH_WT(float) }
    }
#undef LH_WT
    lh_set_error("lh_wgrad: unsupported dtype %d", dtype);
    return LH_ERR_ARG;
}

// Plan, fill and launch one weight gradient into its slab.
static int wgrad_run(const lh_igemm_desc* d, const void* x, const void* dy, int dy_pix_stride, int n_out, int n_in, float* slab,
                     int dtype, void* stream, int fold_rows) {
    // what the planner reads -- the descriptor and its tap list -- is checked here; everything else by wgrad_fill_args
    LH_REQUIRE(d && x && dy && slab, "lh_wgrad: null pointer");
    LH_REQUIRE(d->ntaps > 0 && d->ntaps <= 64, "lh_wgrad: ntaps %d out of range", d->ntaps);
    WgradPlan c;
    WgradArgs a;
    int rc = wgrad_plan(d, n_out, n_in, dtype, &c);
    if (!rc) rc = wgrad_fill_args(d, x, dy, dy_pix_stride, n_out, n_in, slab, dtype, fold_rows, c, &a);
    return rc ? rc : wgrad_launch(a, c, dtype, (hipStream_t)stream);
}

extern "C" int lh_wgrad(const lh_igemm_desc* d, const void* x, const void* dy, int dy_pix_stride,
                        int n_out, int n_in, float* slab, int dtype, void* stream) {
    return wgrad_run(d, x, dy, dy_pix_stride, n_out, n_in, slab, dtype, stream, 0);
}

extern "C" int lh_wgrad_rowfold(const lh_igemm_desc* d, int rows, const void* x, const void* dy, int dy_pix_stride,
                                int n_out, float* slab, int dtype, void* stream) {
    LH_REQUIRE(d && rows >= 1, "lh_wgrad_rowfold: bad arguments");
    return wgrad_run(d, x, dy, dy_pix_stride, n_out, d->k_run, slab, dtype, stream, rows);
}

extern "C" int lh_wgrad_fused(const lh_igemm_desc* d, int rows, const void* x, const void* dy, int dy_pix_stride, int n_out,
                              int n_in, void* workspace, float* grad, long so, long si, long sr, long ss, const int* taps_rs,
                              int accumulate, int dtype, void* stream) {
    LH_REQUIRE(d && workspace && grad && taps_rs, "lh_wgrad_fused: null pointer");
    const int rc = wgrad_run(d, x, dy, dy_pix_stride, n_out, n_in, (float*)workspace, dtype, stream, rows);
    if (rc) return rc;
    return lh_wgrad_reduce(d, (const float*)workspace, grad, n_out, n_in, so, si, sr, ss, taps_rs, accumulate, dtype, stream);
}

extern "C" int lh_wgrad_reduce(const lh_igemm_desc* d, const float* slab, float* grad, int n_out,
                               int n_in, long so, long si, long sr, long ss, const int* taps_rs,
                               int accumulate, int dtype, void* stream) {
    LH_REQUIRE(d && slab && grad && taps_rs, "lh_wgrad_reduce: null pointer");                         // (as in wgrad_run: the planner reads these)
    LH_REQUIRE(d->ntaps > 0 && d->ntaps <= 64, "lh_wgrad_reduce: ntaps %d out of range", d->ntaps);
    WgradPlan c;
    WreduceArgs a;
    int rc = wgrad_plan(d, n_out, n_in, dtype, &c);              // the split count of the launch that wrote the slab
    if (!rc) rc = reduce_prepare(d, slab, grad, n_out, n_in, so, si, sr, ss, taps_rs, accumulate, c.nsplit, &a);
    if (rc) return rc;
    if (a.contig) hipLaunchKernelGGL(wgrad_reduce_contig_kernel, dim3(wgrad_reduce_blocks(a)), dim3(256), wgrad_reduce_lds(a), (hipStream_t)stream, a);
    else hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(wgrad_reduce_blocks(a)), dim3(256), 0, (hipStream_t)stream, a);
    LH_LAUNCH_CHECK("wgrad_reduce launch");
    return LH_OK;
}

// n independent weight gradients (each with its OWN slab workspace) that share tile / stage / ring depth: ONE launch of
// the LDS-DMA kernel for all of them, then ONE launch that folds all their pixel-split slabs (the same layer position of
// HRNet's parallel branches, pose_hrnet.py:139-185).  Problems that need another kernel -- row folds, the register-staged
// kernel, the transposing fold of very large tensors -- run through lh_wgrad_fused one by one.
extern "C" int lh_wgrad_fused_multi(const lh_wgrad_call* calls, int n, int dtype, void* stream) {
    LH_REQUIRE(calls && n >= 1, "lh_wgrad_fused_multi: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    LhMulti<WgradArgs> m;
    LhMulti<WreduceArgs> r;
    WgradPlan plan0 = {0, 0, 0, 0, 0, 0};
    m.n = r.n = 0; m.first[0] = r.first[0] = 0;
    auto flush = [&]() -> int {
        if (m.n == 0) return LH_OK;
        int rc;
        if (m.n > 1) {
            // longest split first: workgroups are dispatched in grid order, and the launch ends with its last one
            int order[LH_MULTI_MAX];
            for (int i = 0; i < m.n; ++i) order[i] = i;
            std::stable_sort(order, order + m.n, [&](int x, int y) { return m.a[x].steps_per_split > m.a[y].steps_per_split; });
            LhMulti<WgradArgs> t = m;
            for (int i = 0; i < m.n; ++i) {
                m.a[i] = t.a[order[i]];
                m.first[i + 1] = m.first[i] + m.a[i].tiles * m.a[i].ntaps * m.a[i].nsplit;
            }
        }
        if (m.n == 1) rc = dtype == LH_BF16 ? lh_wgrad_ring_launch_bf16(m.a[0], plan0, s) : lh_wgrad_ring_launch_f16(m.a[0], plan0, s);
        else rc = dtype == LH_BF16 ? lh_wgrad_ring_multi_launch_bf16(m, plan0, s) : lh_wgrad_ring_multi_launch_f16(m, plan0, s);
        if (rc == 1) {
            lh_set_error("lh_wgrad_fused_multi: no multi-problem kernel for tile %dx%d stage %d depth %d", plan0.bo, plan0.bi, plan0.kps, plan0.depth);
            return LH_ERR_UNSUPPORTED;
        }
        if (rc) return rc;
        if (r.n == 1) hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(r.first[1]), dim3(256), 0, s, r.a[0]);
        else hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3(r.first[r.n]), dim3(256), 0, s, r);
        LH_LAUNCH_CHECK("wgrad_reduce_multi launch");
        m.n = r.n = 0;
        return LH_OK;
    };
    for (int i = 0; i < n; ++i) {
        const lh_wgrad_call& q = calls[i];
        LH_REQUIRE(q.d && q.workspace && q.grad && q.taps_rs, "lh_wgrad_fused_multi: null pointer (problem %d)", i);
        WgradPlan c;
        int rc = wgrad_plan(q.d, q.n_out, q.n_in, dtype, &c);
        if (rc) return rc;
        WreduceArgs ra;
        rc = reduce_prepare(q.d, (const float*)q.workspace, q.grad, q.n_out, q.n_in, q.so, q.si, q.sr, q.ss, q.taps_rs, q.accumulate, c.nsplit, &ra);
        if (rc) return rc;
        const bool batchable = lh_dtype_size(dtype) == 2 && c.kps && q.rows <= 1 && !ra.contig &&
                               (c.bo <= 128 && c.bi <= 128);           // 4-wave tiles only
        const bool same = m.n == 0 || (c.bo == plan0.bo && c.bi == plan0.bi && c.kps == plan0.kps && c.depth == plan0.depth);
        if (!batchable || !same) {
            rc = flush();
            if (rc) return rc;
        }
        if (!batchable) {
            rc = lh_wgrad_fused(q.d, q.rows, q.x, q.dy, q.dy_pix_stride, q.n_out, q.n_in, q.workspace, q.grad, q.so, q.si, q.sr, q.ss, q.taps_rs,
                                q.accumulate, dtype, stream);
            if (rc) return rc;
            continue;
        }
        WgradArgs& a = m.a[m.n];
        rc = wgrad_fill_args(q.d, q.x, q.dy, q.dy_pix_stride, q.n_out, q.n_in, (float*)q.workspace, dtype, 0, c, &a);
        if (rc) return rc;
        a.zero = wgrad_zero_page();
        LH_REQUIRE(a.zero, "lh_wgrad: cannot resolve the zero page on this device");
        if (m.n == 0) plan0 = c;
        m.first[m.n + 1] = m.first[m.n] + a.tiles * a.ntaps * a.nsplit;
        r.a[r.n] = ra;
        r.first[r.n + 1] = r.first[r.n] + wgrad_reduce_blocks(ra);
        ++m.n; ++r.n;
        if (m.n == LH_MULTI_MAX) {
            rc = flush();
            if (rc) return rc;
        }
    }
    return flush();
}
