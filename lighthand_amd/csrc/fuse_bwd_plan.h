// Host side of the fused op's backward (fuse_bwd.hip): a C-ABI call is PLANNED into launch records -- strips of the reduce
// pass, the term's workspace slice, which kernels run -- before anything is launched.
#pragma once
#include "fuse_bwd_kernel.h"
#include <vector>
#include <algorithm>

// Strips of the streaming reduce pass = rows of the partial-sum slab the coefficient fold reads.  Measured on the R50 and
// HRNet-W32 steps: 512 strips for a node that runs alone (1 024: the fold is a longer latency chain, -0.08 ms per step
// for 512; 256: the reduce pass loses occupancy), 256 per node when several nodes share a launch (lh_fuse_bwd_multi;
// the caller says so in lh_fuse_bwd_desc.strips_cap, so that a node plans the same strips alone and in company).
static long fuse_bwd_strips(long count, int* rows_per_strip, int strips_cap = 0) {
    const long cap = strips_cap >= 16 && strips_cap <= 512 ? strips_cap : 512;
    long rps = (count + cap - 1) / cap;
    if (rps < 16) rps = 16;
    *rows_per_strip = (int)rps;
    return (count + rps - 1) / rps;
}

// bytes of ONE term's slice: partial slab + coefficients, rounded to 256.  (The doubles between the two were the column
// sums and totals of a two-stage fold that no longer exists; they stay reserved because the callers lay their memory out
// with lh_fuse_bwd_workspace_bytes.)
static size_t fuse_bwd_term_bytes(int n, int h, int w, int c) {
    int rps;
    const long strips = fuse_bwd_strips((long)n * h * w, &rps);
    const size_t b = (size_t)strips * 2 * c * 4 + 16 + (size_t)(ceil_div(strips, 256) + 1) * 2 * c * 8 + (size_t)4 * c * 4;
    return (b + 255) & ~(size_t)255;
}

// ---- launch records: a C-ABI call is first PLANNED into the kernel launches it consists of (kind, grid, phase, the
// argument block of that kind), then run phase by phase -- the records of a phase, of one call or of several independent
// calls, LH_MULTI_MAX per launch (multi.h).
struct BwdLaunch {
    int kind, grid;
    int phase;                   // 0 reduce, 1 coefficient fold, 2 apply (a pass only depends on the passes of lower phase)
    union {
        FuseBwdArgs fb;          // reduce and one-term apply kinds
        FuseBwd2Args fb2;        // K_FB_APPLY2
        CoefArgs co;             // K_FB_COEF
    };
    static BwdLaunch of(int kind, int grid, int phase, const FuseBwdArgs& a) { BwdLaunch r; r.kind = kind; r.grid = grid; r.phase = phase; r.fb = a; return r; }
    // the gradient buffers an apply record writes (null: that term's gradient is not wanted)
    void dsts(const void* out[2]) const {
        if (kind == K_FB_APPLY2) { out[0] = fb2.dx[0]; out[1] = fb2.dx[1]; }
        else { out[0] = fb.dx; out[1] = nullptr; }
    }
    // an apply record whose kernel ends with lh_l2_touch (the flat ones) takes the bytes to warm
    void set_touch(const void* p, size_t bytes) {
        if (kind == K_FB_APPLY2) { fb2.touch = (const unsigned char*)p; fb2.touch_bytes = (unsigned)bytes; }
        else if (kind == K_FB_APPLY_FLAT || kind == K_FB_APPLY_FLAT_X) { fb.touch = (const unsigned char*)p; fb.touch_bytes = (unsigned)bytes; }
    }
};

// step 1: term t of the descriptor as an argument block (no workspace, no strips yet)
static FuseBwdArgs term_args(const lh_fuse_bwd_desc* d, int t, int n, int h, int w, int c, int nchunk) {
    FuseBwdArgs a{};
    a.dout = (const unsigned char*)d->dout; a.out = (const unsigned char*)d->out;
    a.mask = (const unsigned char*)d->relu_mask;
    a.x = (const unsigned char*)d->x[t]; a.scale = d->scale[t]; a.mean = d->save_mean[t]; a.invstd = d->save_invstd[t];
    a.dx = (unsigned char*)d->dx[t]; a.dgamma = d->dgamma[t]; a.dbeta = d->dbeta[t];
    a.h = h; a.w = w; a.c = c; a.l = d->log2up[t]; a.relu = d->relu; a.accumulate = d->accumulate[t];
    a.count = (long)n * (h >> a.l) * (w >> a.l);
    a.total = a.count * nchunk;
    a.exp = bn_exp_flags() & 3;
    return a;
}

// step 2: dout written by lh_igemm_gated is already the gated gradient and its partial sums come with it
static int check_pre_partial(const lh_fuse_bwd_desc* d, const FuseBwdArgs& a, bool merge2, bool two_bn) {
    // one BatchNorm term under the ReLU, alone or with an identity term beside it (a residual tail, merged apply pass); or a tail
    // with a projection shortcut: two BatchNorm terms, each with its slab
    LH_REQUIRE((d->nterms == 1 || merge2) && d->relu && d->pre_rows >= 1 && a.l == 0 && (a.x || merge2) && (!two_bn || d->pre_partial2),
               "lh_fuse_bwd: pre_partial takes a ReLU node with one BatchNorm term (alone, or beside one identity term) or a two-term tail with pre_partial2");
    return LH_OK;
}

// step 3 of a BatchNorm term: strips of its reduce pass (the caller's rows with pre_slab), whether the apply pass folds
// them itself (a.fold_rows), and the term's slice of the workspace: slab, then -- past the reserve, see
// fuse_bwd_term_bytes -- the coefficients.  Returns the strips.
static long carve_term(const lh_fuse_bwd_desc* d, FuseBwdArgs& a, const float* pre_slab, bool flat, int es, unsigned char* slice, int coef_block) {
    const int c = a.c;
    long strips = fuse_bwd_strips(a.count, &a.rows_per_strip, d->strips_cap);
    // small tensors (HRNet's branches): few enough strips that the apply pass folds them itself; a strip must stay
    // short (<= 64 KiB of the operand), else the reduce pass would lose the workgroups it streams with
    const bool may_fold = flat && c <= 256 && getenv("LH_FOLD_IN_APPLY") == nullptr;
    bool fold_in_apply = false;
    if (pre_slab) {
        strips = d->pre_rows;
        fold_in_apply = may_fold && strips * 2 * c <= LH_FOLD_IN_APPLY_FLOATS;
    } else if (may_fold) {
        int rps2;
        const long s2 = fuse_bwd_strips(a.count, &rps2, (int)std::min<long>(d->strips_cap >= 16 ? d->strips_cap : 512, LH_FOLD_IN_APPLY_FLOATS / (2 * c)));
        if (s2 * 2 * c <= LH_FOLD_IN_APPLY_FLOATS && (long)rps2 * c * es <= 65536) {
            fold_in_apply = true;
            strips = s2;
            a.rows_per_strip = rps2;
        }
    }
    a.fold_rows = fold_in_apply ? (int)strips : 0;
    const long slab_floats = pre_slab ? 0 : strips * 2 * c;      // pre: the slab is the caller's, the workspace holds the coefficients only
    double* reserve = (double*)((float*)slice + ((slab_floats + 3) & ~3L));
    a.partial = pre_slab ? const_cast<float*>(pre_slab) : (float*)slice;
    a.coef = (float*)(reserve + ((long)ceil_div(strips, 256) + 1) * 2 * c) + (size_t)coef_block * 2 * c;
    return strips;
}

// the one pass that writes both gradients of a two-term node, from its finished terms (a term whose gradient is not
// wanted was not planned: a value-initialised block, which the kernel skips)
static FuseBwd2Args merge_terms(const lh_fuse_bwd_desc* d, const FuseBwdArgs term[2], int c, long count, long total) {
    FuseBwd2Args m{};
    const bool gated = d->pre_partial != nullptr;                // dout is the gated gradient already
    m.dout = (const unsigned char*)d->dout;
    m.out = gated ? nullptr : (const unsigned char*)d->out;
    m.mask = gated ? nullptr : (const unsigned char*)d->relu_mask;
    m.relu = gated ? 0 : d->relu;
    m.c = c; m.count = count; m.total = total;
    m.exp = bn_exp_flags() & 3;
    for (int k = 0; k < 2; ++k) {
        const FuseBwdArgs& a = term[k];
        m.x[k] = a.x; m.scale[k] = a.scale; m.mean[k] = a.mean; m.invstd[k] = a.invstd; m.coef[k] = a.coef;
        m.dx[k] = a.dx; m.accumulate[k] = a.accumulate;
        m.fold_slab[k] = a.fold_rows > 0 ? a.partial : nullptr; m.fold_rows[k] = a.fold_rows;
        m.dgamma[k] = a.dgamma; m.dbeta[k] = a.dbeta;
    }
    return m;
}

static int plan_fuse_bwd(const lh_fuse_bwd_desc* d, int n, int h, int w, int c, void* workspace, int dtype, std::vector<BwdLaunch>& v) {
    LH_REQUIRE(d && d->dout && d->nterms >= 1 && d->nterms <= 4, "lh_fuse_bwd: bad descriptor");
    LH_REQUIRE(!d->relu || d->out || d->relu_mask, "lh_fuse_bwd: relu needs the forward output or its mask bits");
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0 && c % (16 / es) == 0, "lh_fuse_bwd: c %d not a multiple of the 16-byte chunk", c);
    const int nchunk = c / (16 / es);
    const bool merge2 = d->nterms == 2 && d->log2up[0] == 0 && d->log2up[1] == 0 && bn_flat_chunks(nchunk) && (d->dx[0] || d->dx[1]);
    const bool two_bn = d->nterms == 2 && d->x[0] && d->x[1];
    const size_t term_bytes = fuse_bwd_term_bytes(n, h, w, c);
    FuseBwdArgs merged[2] = {};
    for (int t = 0; t < d->nterms; ++t) {
        if (!d->dx[t]) continue;
        const int l = d->log2up[t];
        LH_REQUIRE(l >= 0 && (h >> l) << l == h && (w >> l) << l == w, "lh_fuse_bwd: bad upsampling factor");
        FuseBwdArgs a = term_args(d, t, n, h, w, c, nchunk);
        const bool flat = l == 0 && bn_flat_chunks(nchunk);
        const float* pre_slab = !(d->pre_partial && a.x) ? nullptr : (two_bn && t == 1) ? d->pre_partial2 : d->pre_partial;
        if (d->pre_partial) {
            const int rc = check_pre_partial(d, a, merge2, two_bn);
            if (rc) return rc;
            a.relu = 0;
            a.out = nullptr; a.mask = nullptr;
        }
        // single BN term under the ReLU: the mask is sign(x*scale+shift), no need to read the stored activation
        const bool mask_from_x = !pre_slab && flat && d->relu && d->nterms == 1 && a.x && d->shift[t];
        if (mask_from_x) a.shift = d->shift[t];
        LH_REQUIRE((long)n * h * w * nchunk < (1L << 31), "lh_fuse_bwd: tensor too large for 32-bit chunk indices");
        if (a.x) {
            LH_REQUIRE(workspace && a.scale && a.mean && a.invstd, "lh_fuse_bwd: BN term %d lacks workspace/statistics", t);
            // merging keeps one coefficient block per term
            const long strips = carve_term(d, a, pre_slab, flat, es, (unsigned char*)workspace + (size_t)t * term_bytes, merge2 ? t : 0);
            if (!pre_slab)
                v.push_back(BwdLaunch::of(flat ? (mask_from_x ? K_FB_REDUCE_FLAT_X : K_FB_REDUCE_FLAT) : K_FB_REDUCE_GEN, (int)strips, 0, a));
            if (!a.fold_rows) {
                BwdLaunch q;
                q.kind = K_FB_COEF; q.grid = fold_grid((int)strips, c); q.phase = 1;
                q.co = CoefArgs{a.partial, (int)strips, c, a.count, a.coef, a.dgamma, a.dbeta};
                v.push_back(q);
            }
        }
        if (merge2) { merged[t] = a; continue; }     // both gradients are written by ONE pass below
        if (flat) v.push_back(BwdLaunch::of(mask_from_x ? K_FB_APPLY_FLAT_X : K_FB_APPLY_FLAT, flat_grid(a.total), 2, a));      // >= 4 chunks per thread
        else v.push_back(BwdLaunch::of(K_FB_APPLY_GEN, generic_grid(a.total), 2, a));
    }
    if (merge2) {
        BwdLaunch r;
        r.kind = K_FB_APPLY2; r.phase = 2;
        r.fb2 = merge_terms(d, merged, c, (long)n * h * w, (long)n * h * w * nchunk);
        r.grid = flat_grid(r.fb2.total);
        v.push_back(r);
    }
    // the LAST launch of the call (an apply pass) warms what the next launch on the stream reads first (lh_fuse_bwd_desc.l2_touch)
    const unsigned touch = lh_touch_bytes(d->l2_touch, d->l2_touch_bytes);
    if (touch && !v.empty()) v.back().set_touch(d->l2_touch, touch);
    return LH_OK;
}
