// The fused "sum of affine terms (+ nearest upsample) + ReLU" elementwise op, backward: per BatchNorm term a reduce pass
// (partial sums of g and g * xhat), a coefficient fold and an apply pass; one node, or several independent nodes phase by phase.
// The passes are in fuse_bwd_kernel.h, the planner in fuse_bwd_plan.h; here: the mixed kernels, the runner, the entry points.
#include "fuse_bwd_kernel.h"
#include "fuse_bwd_plan.h"

// Reduce / apply passes of DIFFERENT kinds in one grid (the terms of an HRNet exchange sum: BN terms without and with
// upsampling, identity terms): the kind is a per-problem tag next to the argument blocks.
struct KindTags { int k[LH_MULTI_MAX]; };
template <typename T>
__global__ __launch_bounds__(256) void fuse_bwd_reduce_mixed_kernel(const LhMulti<FuseBwdArgs> m, const KindTags kt) {
    int bid, nblk;
    const int i = lh_multi_pick(m, bid, nblk);
    switch (kt.k[i]) {
        case K_FB_REDUCE_GEN: fuse_bwd_reduce<T>::run(m.a[i], bid, nblk); break;
        case K_FB_REDUCE_FLAT: fuse_bwd_reduce_flat<T, false>::run(m.a[i], bid, nblk); break;
        default: fuse_bwd_reduce_flat<T, true>::run(m.a[i], bid, nblk); break;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void fuse_bwd_apply_mixed_kernel(const LhMulti<FuseBwdArgs> m, const KindTags kt) {
    int bid, nblk;
    const int i = lh_multi_pick(m, bid, nblk);
    switch (kt.k[i]) {
        case K_FB_APPLY_GEN: fuse_bwd_apply<T>::run(m.a[i], bid, nblk); break;
        case K_FB_APPLY_FLAT: fuse_bwd_apply_flat<T, false>::run(m.a[i], bid, nblk); break;
        default: fuse_bwd_apply_flat<T, true>::run(m.a[i], bid, nblk); break;
    }
}

// every term of a node owns a slice of the workspace: the terms' passes are independent of each other and run as
// multi-problem launches (all reduce passes, then all coefficient folds, then all apply passes)
extern "C" size_t lh_fuse_bwd_workspace_bytes(int n, int h, int w, int c) { return 4 * fuse_bwd_term_bytes(n, h, w, c); }

// Run n <= LH_MULTI_MAX records of ONE kind: a plain launch for one, a multi-problem launch for several.
static int bn_run(const BwdLaunch* const* L, int n, int dtype, hipStream_t s) {
    LH_REQUIRE(n >= 1 && n <= LH_MULTI_MAX, "bn_run: %d records", n);
    switch (L[0]->kind) {
        case K_FB_REDUCE_GEN: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_reduce<T>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_REDUCE_FLAT: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_reduce_flat<T, false>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_REDUCE_FLAT_X: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_reduce_flat<T, true>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_COEF: lh_launch_records<fuse_bwd_coef_fused>(L, n, &BwdLaunch::co, s); break;
        case K_FB_APPLY_GEN: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_apply<T>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_APPLY_FLAT: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_apply_flat<T, false>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_APPLY_FLAT_X: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_apply_flat<T, true>>(L, n, &BwdLaunch::fb, s)); break;
        case K_FB_APPLY2: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_bwd_apply2_flat<T>>(L, n, &BwdLaunch::fb2, s)); break;
        default: lh_set_error("bn_run: unknown kind %d", L[0]->kind); return LH_ERR_ARG;
    }
    LH_LAUNCH_CHECK("BatchNorm / ReLU pass launch");
    return LH_OK;
}

static int bn_run_mixed(const BwdLaunch* const* L, int n, int dtype, hipStream_t s) {
    LhMulti<FuseBwdArgs> m;
    KindTags kt;
    m.n = n; m.first[0] = 0;
    for (int i = 0; i < n; ++i) { m.a[i] = L[i]->fb; kt.k[i] = L[i]->kind; m.first[i + 1] = m.first[i] + L[i]->grid; }
    for (int i = n; i < LH_MULTI_MAX; ++i) kt.k[i] = 0;
    if (L[0]->phase == 0) { LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((fuse_bwd_reduce_mixed_kernel<T>), dim3(m.first[n]), dim3(256), 0, s, m, kt)); }
    else { LH_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((fuse_bwd_apply_mixed_kernel<T>), dim3(m.first[n]), dim3(256), 0, s, m, kt)); }
    LH_LAUNCH_CHECK("BatchNorm / ReLU mixed pass launch");
    return LH_OK;
}

// n records, `per` of them per launch: through their kind's kernel when the records of a launch agree in kind, else
// through the mixed kernel of their phase
static int bn_run_chunks(const BwdLaunch* const* L, size_t n, size_t per, int dtype, hipStream_t s) {
    for (size_t i = 0; i < n; i += per) {
        const int m = (int)std::min(n - i, per);
        bool one = true;
        for (int k = 1; k < m; ++k) one = one && L[i + k]->kind == L[i]->kind;
        const int rc = one ? bn_run(L + i, m, dtype, s) : bn_run_mixed(L + i, m, dtype, s);
        if (rc) return rc;
    }
    return LH_OK;
}

// The backward passes of n planned calls, phase by phase (all reduce passes, all coefficient folds, all apply passes):
// inside a phase the passes are independent -- every term has its own workspace slice and its own gradient -- so they
// run LH_MULTI_MAX per launch, passes of one kind through that kind's kernel, the rest through the mixed kernels.
static int bn_run_phases(const std::vector<std::vector<BwdLaunch>>& plans, int dtype, hipStream_t s) {
    // two passes that write ONE gradient buffer (an activation that enters a node twice) must keep their recorded order
    std::vector<const BwdLaunch*> all;
    std::vector<const void*> dsts;
    for (const auto& pl : plans)
        for (const BwdLaunch& r : pl) {
            all.push_back(&r);
            if (r.phase != 2) continue;
            const void* d[2];
            r.dsts(d);
            for (const void* q : d) if (q) dsts.push_back(q);
        }
    std::sort(dsts.begin(), dsts.end());
    if (std::adjacent_find(dsts.begin(), dsts.end()) != dsts.end()) return bn_run_chunks(all.data(), all.size(), 1, dtype, s);
    for (int phase = 0; phase < 3; ++phase) {
        std::vector<const BwdLaunch*> by_kind[K_FB_APPLY2 + 1], rest;
        for (const BwdLaunch* r : all) if (r->phase == phase) by_kind[r->kind].push_back(r);
        // FuseBwdArgs reduce / apply passes: whole groups of one kind first (their own kernels, no kind switch), what is
        // left over goes to the mixed kernel; then the coefficient folds and the two-term applies, each by kind
        for (int kind = K_FB_REDUCE_GEN; kind <= K_FB_APPLY2; ++kind) {
            if (kind == K_FB_COEF || kind == K_FB_APPLY2) continue;
            const std::vector<const BwdLaunch*>& same = by_kind[kind];
            const size_t whole = same.size() / LH_MULTI_MAX * LH_MULTI_MAX;
            const int rc = bn_run_chunks(same.data(), whole, LH_MULTI_MAX, dtype, s);
            if (rc) return rc;
            rest.insert(rest.end(), same.begin() + whole, same.end());
        }
        for (const std::vector<const BwdLaunch*>* g : {&rest, &by_kind[K_FB_COEF], &by_kind[K_FB_APPLY2]}) {
            const int rc = bn_run_chunks(g->data(), g->size(), LH_MULTI_MAX, dtype, s);
            if (rc) return rc;
        }
    }
    return LH_OK;
}

extern "C" int lh_fuse_bwd(const lh_fuse_bwd_desc* d, int n, int h, int w, int c, void* workspace, int dtype,
                           void* stream) {
    std::vector<std::vector<BwdLaunch>> plans(1);
    const int rc = plan_fuse_bwd(d, n, h, w, c, workspace, dtype, plans[0]);
    if (rc) return rc;
    return bn_run_phases(plans, dtype, (hipStream_t)stream);
}

// the published kind values (include/lighthand_hip.h) are the planner's
static_assert(LH_FB_REDUCE_GEN == K_FB_REDUCE_GEN, "LH_FB_REDUCE_GEN");
static_assert(LH_FB_REDUCE_FLAT == K_FB_REDUCE_FLAT, "LH_FB_REDUCE_FLAT");
static_assert(LH_FB_REDUCE_FLAT_X == K_FB_REDUCE_FLAT_X, "LH_FB_REDUCE_FLAT_X");
static_assert(LH_FB_COEF == K_FB_COEF, "LH_FB_COEF");
static_assert(LH_FB_APPLY_GEN == K_FB_APPLY_GEN, "LH_FB_APPLY_GEN");
static_assert(LH_FB_APPLY_FLAT == K_FB_APPLY_FLAT, "LH_FB_APPLY_FLAT");
static_assert(LH_FB_APPLY_FLAT_X == K_FB_APPLY_FLAT_X, "LH_FB_APPLY_FLAT_X");
static_assert(LH_FB_APPLY2 == K_FB_APPLY2, "LH_FB_APPLY2");

// What lh_fuse_bwd would launch for these arguments, in recorded order; nothing is launched (host arithmetic only).
extern "C" int lh_fuse_bwd_plan(const lh_fuse_bwd_desc* d, int n, int h, int w, int c, void* workspace, int dtype, int* kinds,
                                int* grids, int* fold_rows, int cap) {
    std::vector<BwdLaunch> v;
    const int rc = plan_fuse_bwd(d, n, h, w, c, workspace, dtype, v);
    if (rc) return rc;
    for (int i = 0; i < (int)v.size() && i < cap; ++i) {
        if (kinds) kinds[i] = v[i].kind;
        if (grids) grids[i] = v[i].grid;
        if (fold_rows) fold_rows[i] = v[i].kind == K_FB_COEF || v[i].kind == K_FB_APPLY2 ? 0 : v[i].fb.fold_rows;
    }
    return (int)v.size();
}

// n independent nodes (each with its OWN workspace): reduce / coefficient fold / apply of all of them as three launches.
extern "C" int lh_fuse_bwd_multi(const lh_fuse_bwd_call* calls, int n, int dtype, void* stream) {
    LH_REQUIRE(calls && n >= 1, "lh_fuse_bwd_multi: bad arguments");
    std::vector<std::vector<BwdLaunch>> plans(n);
    for (int i = 0; i < n; ++i) {
        const int rc = plan_fuse_bwd(calls[i].d, calls[i].n, calls[i].h, calls[i].w, calls[i].c, calls[i].workspace, dtype, plans[i]);
        if (rc) return rc;
    }
    return bn_run_phases(plans, dtype, (hipStream_t)stream);
}
