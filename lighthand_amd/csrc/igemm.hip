// The launching entry points of the forward / data-gradient convolution: lh_igemm, lh_igemm_gated, lh_igemm_multi, lh_igemm_phases and
// lh_igemm_phases_head (include/lighthand_hip.h).
//
//   out[pixel][co] = sum_{tap} sum_{k < k_run} in[pix(pixel, tap)][k] * wpack[co][tap][k]
//
// Each is the same few steps: prepare() validates the descriptor, fills the kernel-argument block and resolves the launch (ConvPlan:
// kernel + configuration, igemm_plan.hip); attach_gate / attach_phases / attach_head add what the entry point is about; lh_conv_launch
// (igemm_ring.hip) runs the kernel the plan names.
#include "common.h"
#include <algorithm>

#include "igemm_args.h"
#include "multi.h"

// `q` = the descriptor and the pointers of one lh_igemm call
static int prepare(const lh_igemm_call& q, int dtype, bool has_head, IgemmArgs* out, ConvPlan* plan) {
    const lh_igemm_desc* d = q.d;
    LH_REQUIRE(d && q.in && q.wpack && (q.out || has_head), "lh_igemm: null pointer");
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0, "lh_igemm: bad dtype %d", dtype);
    const int epc = 16 / es;
    LH_REQUIRE(d->ntaps >= 0 && d->ntaps <= 64, "lh_igemm: ntaps %d out of range", d->ntaps);
    LH_REQUIRE(d->k_run > 0 && d->k_run % epc == 0, "lh_igemm: k_run %d must be a multiple of %d", d->k_run, epc);
    LH_REQUIRE(d->cout > 0 && d->cout % epc == 0, "lh_igemm: cout %d must be a multiple of %d", d->cout, epc);
    LH_REQUIRE(d->out_pix_stride % epc == 0 && d->out_pix_stride >= d->cout, "lh_igemm: bad out_pix_stride %d", d->out_pix_stride);
    LH_REQUIRE(d->in_pix_stride > 0 && (d->in_pix_stride * es) % 4 == 0, "lh_igemm: bad in_pix_stride");
    LH_REQUIRE(d->n > 0 && d->ho > 0 && d->wo > 0 && d->hi > 0 && d->wi > 0, "lh_igemm: bad sizes");
    LH_REQUIRE((d->ho - 1) * d->osh + d->ooh < d->OH && (d->wo - 1) * d->osw + d->oow < d->OW && d->ooh >= 0 && d->oow >= 0,
               "lh_igemm: output placement exceeds the %dx%d image", d->OH, d->OW);
    LH_REQUIRE(!q.addend_mask || (q.addend && d->out_pix_stride == d->cout), "lh_igemm: addend_mask needs an addend and a dense output (mask bits index 16-byte chunks)");
    LH_REQUIRE((q.scale == nullptr) == (q.shift == nullptr), "lh_igemm: scale and shift must come together");
    if (int rc = lh_conv_plan(d, dtype, plan)) return rc;

    IgemmArgs a = {};                   // no gate, no head, no phases; the device pages are the launch's business
    a.in = (const unsigned char*)q.in; a.w = (const unsigned char*)q.wpack; a.out = (unsigned char*)q.out;
    a.addend = (const unsigned char*)q.addend; a.addend_mask = (const unsigned char*)q.addend_mask;
    a.bias = q.bias; a.scale = q.scale; a.shift = q.shift; a.stats = q.stats;
    a.n = d->n; a.hi = d->hi; a.wi = d->wi; a.in_pix_stride = d->in_pix_stride; a.k_run = d->k_run;
    a.kpad = (d->k_run * es + 127) / 128 * (128 / es);
    a.ho = d->ho; a.wo = d->wo; a.M = d->n * d->ho * d->wo; a.sh = d->sh; a.sw = d->sw; a.cout = d->cout;
    a.OH = d->OH; a.OW = d->OW; a.osh = d->osh; a.osw = d->osw; a.ooh = d->ooh; a.oow = d->oow;
    a.out_pix_stride = d->out_pix_stride; a.ntaps = d->ntaps; a.relu = d->relu;
    for (int i = 0; i < 64; ++i) { a.dh[i] = d->dh[i]; a.dw[i] = d->dw[i]; }
    a.xcd = 1;
    a.nphase = 1;
    a.tw = 1;
    if (plan->kind != LH_CONV_STAGED) lh_tap_grid(d, &a.tw, &a.dh0, &a.dhs, &a.dw0, &a.dws);
    a.kspt = ceil_div(d->k_run * es, plan->kind == LH_CONV_STAGED ? 64 : plan->cfg.kb);      // K steps per tap
    *out = a;
    return LH_OK;
}

// lh_igemm_gated: the launch's output is the gradient of relu(BN(gate.x)) -- the epilogue gates it and writes the partial sums
static int attach_gate(IgemmArgs& a, const lh_igemm_desc* d, const lh_bn_bwd_gate* gate, const ConvPlan& p, int dtype) {
    LH_REQUIRE(gate->x && gate->mean && gate->invstd && gate->partial && (gate->mask || (gate->scale && gate->shift)),
               "lh_igemm_gated: null pointer in the gate (the sign of the activation comes from scale + shift or from mask)");
    LH_REQUIRE(!a.bias && !a.scale && !d->relu && a.nphase == 1 && !a.head_w, "lh_igemm_gated: a data gradient carries no bias / affine / ReLU / phases");
    LH_REQUIRE(!gate->mask || d->out_pix_stride == d->cout, "lh_igemm_gated: gate.mask needs a dense output (mask bits index 16-byte chunks)");
    a.gx = (const unsigned char*)gate->x; a.gmean = gate->mean; a.ginv = gate->invstd; a.gscale = gate->scale; a.gshift = gate->shift;
    a.gmask = (const unsigned char*)gate->mask;
    a.stats = gate->partial;
    if (gate->x2) {
        LH_REQUIRE(gate->mask && gate->mean2 && gate->invstd2 && gate->partial2, "lh_igemm_gated: a second BatchNorm term (x2) needs mask, mean2, invstd2, partial2");
        a.gx2 = (const unsigned char*)gate->x2; a.gmean2 = gate->mean2; a.ginv2 = gate->invstd2; a.stats2 = gate->partial2;
    }
    if (!(lh_kind_gated(p.kind) && lh_dtype_size(dtype) == 2)) {
        lh_set_error("lh_igemm_gated: the launch runs neither on a tiled LDS-DMA configuration nor on a persistent kernel (ring depth %d)", p.cfg.depth);
        return LH_ERR_UNSUPPORTED;
    }
    if (gate->x2 && !lh_kind_gates_two(p.kind)) {
        lh_set_error("lh_igemm_gated: two BatchNorm terms are gated by the pointwise kernel only (ring depth %d)", p.cfg.depth);
        return LH_ERR_UNSUPPORTED;
    }
    return LH_OK;
}

// lh_igemm_phases: the launch prepared for descs[lead] becomes one grid over all phases
static int attach_phases(IgemmArgs& a, const ConvPlan& p, const lh_igemm_desc* const* descs, const void* const* wpacks, int nphase) {
    LH_REQUIRE(!lh_kind_persistent(p.kind), "lh_igemm_phases: the persistent kernels take single launches only");
    LH_REQUIRE(p.kind != LH_CONV_STAGED, "lh_igemm_phases: the form is not supported by the LDS-DMA kernel");
    a.nphase = nphase;
    a.phase_blocks = ceil_div(a.M, p.cfg.bp) * ceil_div(a.cout, p.cfg.bm);
    for (int i = 0; i < nphase; ++i) {
        const lh_igemm_desc* q = descs[i];
        a.ph_w[i] = (const unsigned char*)wpacks[i];
        a.ph_ntaps[i] = q->ntaps; a.ph_tw[i] = 1; a.ph_dh0[i] = a.ph_dhs[i] = a.ph_dw0[i] = a.ph_dws[i] = 0;
        if (q->ntaps > 0)
            LH_REQUIRE(lh_tap_grid(q, &a.ph_tw[i], &a.ph_dh0[i], &a.ph_dhs[i], &a.ph_dw0[i], &a.ph_dws[i]) && a.ph_w[i],
                       "lh_igemm_phases: phase %d has an irregular tap list or no weights", i);
        a.ph_ooh[i] = q->ooh; a.ph_oow[i] = q->oow;
        a.ph_row0[i] = i * ceil_div(a.M, p.cfg.bp);
    }
    return LH_OK;
}

// lh_igemm_phases_head: the 1x1 head applied to every tile inside the epilogue
static int attach_head(IgemmArgs& a, const ConvPlan& p, const lh_head* head, int es) {
    const bool ring = p.kind != LH_CONV_STAGED;
    const int bm = p.cfg.bm, bp = p.cfg.bp;
    LH_REQUIRE(head->w && head->out && head->n_out >= 1 && head->n_out <= 32 && head->w_row_bytes >= a.cout * es,
               "lh_igemm_phases_head: bad head (1..32 output channels, K-major weight rows)");
    LH_REQUIRE(ring && es == 2 && bm == 256 && bp == 256 && a.cout <= 256 && !a.addend && !a.stats,
               "lh_igemm_phases_head: needs the 256 x 256 tile of the LDS-DMA kernel (cfg), a 16-bit type, <= 256 channels, no addend / statistics");
    a.head_w = (const unsigned char*)head->w; a.head_bias = head->bias; a.head_out = head->out;
    a.head_j = head->n_out; a.head_wstride = (int)head->w_row_bytes;
    return LH_OK;
}

extern "C" int lh_igemm(const lh_igemm_desc* d, const void* in, const void* wpack, void* out,
                        const void* addend, const void* addend_mask, const float* bias, const float* scale, const float* shift,
                        float* stats, int dtype, void* stream) {
    IgemmArgs a;
    ConvPlan p;
    if (int rc = prepare({d, in, wpack, out, addend, addend_mask, bias, scale, shift, stats}, dtype, false, &a, &p)) return rc;
    return lh_conv_launch(a, p, dtype, (hipStream_t)stream);
}

extern "C" int lh_igemm_gated(const lh_igemm_desc* d, const void* in, const void* wpack, void* out, const void* addend, const void* addend_mask,
                              const lh_bn_bwd_gate* gate, int dtype, void* stream) {
    LH_REQUIRE(gate, "lh_igemm_gated: null gate");
    IgemmArgs a;
    ConvPlan p;
    if (int rc = prepare({d, in, wpack, out, addend, addend_mask, nullptr, nullptr, nullptr, nullptr}, dtype, false, &a, &p)) return rc;
    if (int rc = attach_gate(a, d, gate, p, dtype)) return rc;
    return lh_conv_launch(a, p, dtype, (hipStream_t)stream);
}

// n independent convolutions that share ONE kernel configuration (every descriptor's cfg names the same tiled
// configuration of the LDS-DMA kernel) as one grid: the same layer position of HRNet's parallel branches
// (pose_hrnet.py:139-185).  Groups of LH_MULTI_MAX problems per launch.
extern "C" int lh_igemm_multi(const lh_igemm_call* calls, int n, int dtype, void* stream) {
    LH_REQUIRE(calls && n >= 1, "lh_igemm_multi: bad arguments");
    for (int i0 = 0; i0 < n; i0 += LH_MULTI_MAX) {
        const int cnt = n - i0 < LH_MULTI_MAX ? n - i0 : LH_MULTI_MAX;
        LhMulti<IgemmArgs> m;
        IgemmArgs tmp[LH_MULTI_MAX];
        ConvPlan plans[LH_MULTI_MAX];
        RingCfg cfg0 = {0, 0, 0, 0};                 // the tiled configuration of the call (its ring members share it)
        int ndirect = 0;
        m.n = cnt; m.first[0] = 0;
        for (int i = 0; i < cnt; ++i) {
            if (int rc = prepare(calls[i0 + i], dtype, false, &tmp[i], &plans[i])) return rc;
            const RingCfg& c = plans[i].cfg;
            // (a dense-wave form is a configuration of the LDS-DMA kernel like any other: it passes here, and a call of several such
            //  members ends where the 256-wide tiles do -- no multi-problem kernel, LH_ERR_UNSUPPORTED; a lone one runs its own kernel)
            LH_REQUIRE(plans[i].kind == LH_CONV_TILED || plans[i].kind == LH_CONV_DENSE || plans[i].kind == LH_CONV_DIRECT,
                       "lh_igemm_multi: problem does not run on the LDS-DMA ring kernel or the direct 3x3 kernel (its cfg must name a tiled or the direct configuration)");
            if (plans[i].kind == LH_CONV_DIRECT) { ++ndirect; continue; }
            if (cfg0.bm == 0) cfg0 = c;
            LH_REQUIRE(c.bm == cfg0.bm && c.bp == cfg0.bp && c.depth == cfg0.depth && c.kb == cfg0.kb,
                       "lh_igemm_multi: problem %d runs tile %dx%d depth %d kb %d, another %dx%d depth %d kb %d -- one tiled configuration per call",
                       i0 + i, c.bm, c.bp, c.depth, c.kb, cfg0.bm, cfg0.bp, cfg0.depth, cfg0.kb);
        }
        if (cnt == 1) {                              // a lone problem, tiled or direct: its own kernel
            if (int rc = lh_conv_launch(tmp[0], plans[0], dtype, (hipStream_t)stream)) return rc;
            continue;
        }
        if (ndirect) {
            // (round 4's mixed launch -- direct 3x3 bodies beside ring tiles in one grid -- was measured slower and removed in round 6)
            lh_set_error("lh_igemm_multi: direct 3x3 problems do not share a launch with tiled ones (launch them one by one)");
            return LH_ERR_UNSUPPORTED;
        }
        // longest K loop first: workgroups are dispatched in grid order, so the problem whose tiles take longest must not
        // be the one that starts last (the launch ends with its last tile)
        int order[LH_MULTI_MAX];
        for (int i = 0; i < cnt; ++i) order[i] = i;
        std::stable_sort(order, order + cnt, [&](int x, int y) { return tmp[x].ntaps * tmp[x].kspt > tmp[y].ntaps * tmp[y].kspt; });
        for (int i = 0; i < cnt; ++i) {
            m.a[i] = tmp[order[i]];
            m.first[i + 1] = m.first[i] + ceil_div(m.a[i].M, cfg0.bp) * ceil_div(m.a[i].cout, cfg0.bm);
        }
        if (int rc = lh_igemm_ring_multi_launch(m, cfg0, dtype, (hipStream_t)stream)) return rc;
    }
    return LH_OK;
}

// ---- phase batching ------------------------------------------------------------------------------------------------
extern "C" int lh_igemm_phases(const lh_igemm_desc* const* descs, int nphase, const void* in, const void* const* wpacks,
                               void* out, const void* addend, const void* addend_mask, const float* bias, const float* scale,
                               const float* shift, float* stats, int dtype, void* stream) {
    LH_REQUIRE(lh_phases_ok(descs, nphase) && wpacks, "lh_igemm_phases: 2..4 descriptors that differ only in taps / placement are required");
    const int lead = lh_phase_lead(descs, nphase);
    LH_REQUIRE(descs[lead]->ntaps > 0 && wpacks[lead], "lh_igemm_phases: no phase has taps");
    IgemmArgs a;
    ConvPlan p;
    if (int rc = prepare({descs[lead], in, wpacks[lead], out, addend, addend_mask, bias, scale, shift, stats}, dtype, false, &a, &p)) return rc;
    if (int rc = attach_phases(a, p, descs, wpacks, nphase)) return rc;
    return lh_conv_launch(a, p, dtype, (hipStream_t)stream);
}

// The phases of a transposed convolution + per-channel affine + ReLU + a 1x1 head in ONE launch (include/lighthand_hip.h).
extern "C" int lh_igemm_phases_head(const lh_igemm_desc* const* descs, int nphase, const void* in, const void* const* wpacks,
                                    const float* scale, const float* shift, const lh_head* head, int dtype, void* stream) {
    LH_REQUIRE(lh_phases_ok(descs, nphase) && wpacks && head, "lh_igemm_phases_head: 2..4 descriptors that differ only in taps / placement are required");
    const int lead = lh_phase_lead(descs, nphase);
    LH_REQUIRE(descs[lead]->ntaps > 0 && wpacks[lead], "lh_igemm_phases_head: no phase has taps");
    IgemmArgs a;
    ConvPlan p;
    if (int rc = prepare({descs[lead], in, wpacks[lead], nullptr, nullptr, nullptr, nullptr, scale, shift, nullptr}, dtype, true, &a, &p)) return rc;
    if (int rc = attach_phases(a, p, descs, wpacks, nphase)) return rc;
    if (int rc = attach_head(a, p, head, lh_dtype_size(dtype))) return rc;
    return lh_conv_launch(a, p, dtype, (hipStream_t)stream);
}
