// Host arithmetic of the forward / data-gradient convolution, no launches: which kernel configurations exist, which of them fit a
// launch, the static default, the ONE resolver (lh_conv_plan), the candidate list, the slab rows -- and the query entry points of
// include/lighthand_hip.h that answer from them.
#include "common.h"

#include "igemm_args.h"
#include "igemm_pw_cfgs.h"
#include <stdlib.h>

int lh_pw_occ_bf16(const RingCfg& c, int mode);
int lh_pw_occ_f16(const RingCfg& c, int mode);

static const RingCfg kCfg16[] = {
#define X(BM, BP, WC, WP, D, KB) {BM, BP, D, KB},
    LH_RING_CFGS_16BIT(X)
#undef X
#define X(BM, BP, WC, WP, D, KB) {BM, BP, D + LH_DENSE_DEPTH, KB},
    LH_RING_CFGS_DENSE(X)
#undef X
};
static const RingCfg kCfg32[] = {
#define X(BM, BP, WC, WP, D, KB) {BM, BP, D, KB},
    LH_RING_CFGS_F32(X)
#undef X
};

struct PwCfg { int bm, kc, pt; };
static const PwCfg kCfgPw[] = {
#define X(BM, KC, PT) {BM, KC, PT},
    LH_PW_CFGS(X)
#undef X
};

static void cfg_table(int dtype, const RingCfg** t, int* n) {
    if (dtype == LH_F32) { *t = kCfg32; *n = (int)(sizeof(kCfg32) / sizeof(RingCfg)); }
    else { *t = kCfg16; *n = (int)(sizeof(kCfg16) / sizeof(RingCfg)); }
}

static bool cfg_exists(int dtype, const RingCfg& c) {
    const RingCfg* t; int n;
    cfg_table(dtype, &t, &n);
    for (int i = 0; i < n; ++i)
        if (t[i].bm == c.bm && t[i].bp == c.bp && t[i].depth == c.depth && t[i].kb == c.kb) return true;
    return false;
}

// Taps of every convolution form on this path are a regular grid: tap t = (t / tw, t % tw) with
// dh = dh0 + (t / tw) * dhs, dw = dw0 + (t % tw) * dws.  Returns false for an irregular list.
bool lh_tap_grid(const lh_igemm_desc* d, int* tw, int* dh0, int* dhs, int* dw0, int* dws) {
    const int n = d->ntaps;
    if (n <= 0) return false;
    int w = 1;
    while (w < n && d->dh[w] == d->dh[0]) ++w;
    if (n % w) return false;
    *tw = w; *dh0 = d->dh[0]; *dw0 = d->dw[0];
    *dws = w > 1 ? d->dw[1] - d->dw[0] : 0;
    *dhs = n > w ? d->dh[w] - d->dh[0] : 0;
    for (int t = 0; t < n; ++t)
        if (d->dh[t] != *dh0 + (t / w) * *dhs || d->dw[t] != *dw0 + (t % w) * *dws) return false;
    return true;
}

// LDS-DMA moves 16 bytes per lane, so every (pixel, tap) row start must be 16-byte aligned: either the pixel rows
// themselves are (C_in * elt % 16 == 0), or -- the NHWC4 stem, 8-byte pixels -- the horizontal stride, the image row
// pitch and every tap's column offset are each a multiple of 16 bytes (7x7/s2 with row taps: 2 pixels per step).
bool lh_ring_supported(const lh_igemm_desc* d, int dtype) {
    const int es = lh_dtype_size(dtype);
    int tw, dh0, dhs, dw0, dws;
    if (d->ntaps <= 0 || d->ntaps > 32 || !lh_tap_grid(d, &tw, &dh0, &dhs, &dw0, &dws)) return false;     // per-lane tap mask: 32 bits
    const long ps = (long)d->in_pix_stride * es;
    if (ps % 16 == 0) return true;
    return (ps * d->sw) % 16 == 0 && (ps * d->wi) % 16 == 0 && (ps * dw0) % 16 == 0 && (ps * dws) % 16 == 0;
}

// A configuration fits a launch when its tile is not wider than the problem rounded up to the smallest tile
// (a 128-channel tile on <= 64 output channels only multiplies zeros) and its ring is not deeper than the K loop.
// Hard rules (an explicit lh_igemm_desc.cfg is refused when it breaks one): what the kernel's loads assume about the pack.
static bool cfg_safe(const lh_igemm_desc* d, int dtype, const RingCfg& c) {
    const int es = lh_dtype_size(dtype);
    if (c.bm == 256 && ((d->cout + 127) / 128) % 2 != 0) return false;   // weight packs are padded to 128 rows, not 256
    if (c.kb == 128 && d->k_run * es <= 64) return false;            // the second K slice would be all padding
    return true;
}

static bool cfg_fits(const lh_igemm_desc* d, int dtype, const RingCfg& c) {
    const int es = lh_dtype_size(dtype);
    const long M = (long)d->n * d->ho * d->wo;
    const int stages = d->ntaps * ((d->k_run * es + c.kb - 1) / c.kb);
    if (!cfg_safe(d, dtype, c)) return false;
    if (c.bm > 64 && d->cout <= c.bm / 2) return false;               // (these three only multiply zeros / repeat a shallower ring)
    if (c.bp > 64 && M <= c.bp / 2) return false;
    if (lh_ring_depth(c) > 2 && lh_ring_depth(c) - 1 > stages) return false;
    // dense-wave forms (LH_DENSE_TILES=0: not offered).  Built for launches that leave a CU one workgroup; measured 2-9 % ahead
    // on larger launches as well (two co-resident workgroups = four waves per SIMD), so every launch is offered them
    if (lh_conv_kind(c.depth) == LH_CONV_DENSE) {
        const char* sw = getenv("LH_DENSE_TILES");
        if (sw && atoi(sw) == 0) return false;
    }
    return true;
}

// ---- persistent pointwise kernel (igemm_pw_kernel.h): one tap at (0, 0), dense output, K <= 512, 16-bit types
static bool pw_supported(const lh_igemm_desc* d, int dtype) {
    if (lh_dtype_size(dtype) != 2) return false;
    if (d->ntaps != 1 || d->dh[0] != 0 || d->dw[0] != 0) return false;
    if (d->osh != 1 || d->osw != 1 || d->OH != d->ho || d->OW != d->wo || d->ooh != 0 || d->oow != 0) return false;
    if (d->k_run > 512 || d->k_run % 8 != 0 || (d->in_pix_stride * 2) % 16 != 0) return false;
    return true;
}

static int pw_kc(const lh_igemm_desc* d) { return d->k_run <= 64 ? 64 : d->k_run <= 128 ? 128 : d->k_run <= 256 ? 256 : 512; }

static bool pw_fits(const lh_igemm_desc* d, int dtype, const RingCfg& c) {
    if (!pw_supported(d, dtype) || c.kb != pw_kc(d)) return false;
    if (c.bm > 64 && d->cout <= c.bm / 2) return false;
    for (const PwCfg& k : kCfgPw)
        if (k.bm == c.bm && k.kc == c.kb && 16 * k.pt == c.bp) return true;
    return false;
}

int lh_pw_occupancy(const RingCfg& c, int dtype, int mode) {
    return dtype == LH_BF16 ? lh_pw_occ_bf16(c, mode) : lh_pw_occ_f16(c, mode);
}

// rows of the statistics slab a pointwise launch writes: one per workgroup of a channel block
static int pw_rows(const lh_igemm_desc* d, const RingCfg& c, int dtype, int gate) {
    int g, cb;
    lh_pw_grid(c.bm, c.kb, c.bp / 16, (long)d->n * d->ho * d->wo, d->cout, lh_pw_occupancy(c, dtype, 1 + gate), &g, &cb);
    return g;
}

// ---- direct 3x3 kernel (conv3x3_direct_kernel.h): nine taps (-1..1)^2 in either order, stride 1, same-size dense output,
//      32 or 64 input channels per tap, 16-bit types
static bool d3_supported(const lh_igemm_desc* d, int dtype) {
    if (lh_dtype_size(dtype) != 2 || d->ntaps != 9) return false;
    if (d->k_run != 32 && d->k_run != 64) return false;
    if (d->sh != 1 || d->sw != 1 || d->hi != d->ho || d->wi != d->wo) return false;
    if (d->osh != 1 || d->osw != 1 || d->OH != d->ho || d->OW != d->wo || d->ooh != 0 || d->oow != 0) return false;
    if ((d->in_pix_stride * 2) % 16 != 0) return false;
    unsigned seen = 0;
    for (int t = 0; t < 9; ++t) {
        if (d->dh[t] < -1 || d->dh[t] > 1 || d->dw[t] < -1 || d->dw[t] > 1) return false;
        seen |= 1u << ((d->dh[t] + 1) * 3 + d->dw[t] + 1);
    }
    return seen == 0x1ffu;
}

static bool d3_fits(const lh_igemm_desc* d, int dtype, const RingCfg& c) {
    return d3_supported(d, dtype) && c.bm == 64 && c.bp == 256 && c.kb == d->k_run;
}

static int d3_rows(const lh_igemm_desc* d) {
    const int cb = (d->cout + 63) / 64;
    const int patch = 18 * 18 * d->k_run * 2, stg = 8 * 2 * 16 * 136;
    const int lds = 9 * 64 * d->k_run * 2 + 2 * patch + (stg <= patch ? 0 : stg) + 512;
    const int occ = lds <= 80 * 1024 ? 2 : 1;
    const long ntile = (long)d->n * ((d->ho + 15) / 16) * ((d->wo + 15) / 16);
    long g = 256L * occ / cb / 8 * 8;
    const long need = (ntile + 7) / 8 * 8;
    if (g > need) g = need;
    if (g < 8) g = 8;
    return (int)g;
}

// Static default (cfg all zero): the largest tile that still gives >= 2 workgroups per CU, a 2-stage ring for K loops
// of <= 4 steps (store-bound 1x1 convolutions: 4 workgroups share a CU) else 4 stages, no look-ahead.  The plan's
// autotuner replaces this by a measured choice (lh_igemm_candidates).
static void default_cfg(const lh_igemm_desc* d, int dtype, RingCfg* out) {
    const long M = (long)d->n * d->ho * d->wo;
    const int es = lh_dtype_size(dtype);
    const int steps = d->ntaps * ((d->k_run * es + 63) / 64);
    const bool f32 = dtype == LH_F32;
    out->kb = 64;
    if (!f32 && d->cout % 256 == 0 && steps > 4 && ((M + 255) / 256) * (d->cout / 256) >= 256) {
        out->bm = 256; out->bp = 256; out->depth = 3;
        return;
    }
    const int cands[5][2] = {{128, 256}, {128, 128}, {128, 64}, {64, 128}, {64, 64}};
    int bm = 64, bp = 64;
    for (int i = 0; i < 5; ++i) {
        const int BM = cands[i][0], BP = cands[i][1];
        if (BM == 128 && d->cout <= 64) continue;
        if (BP == 256 && (f32 || steps <= 4)) continue;                 // 16-bit, deep K only
        if (f32 && BM == 128 && BP == 128) continue;                    // fp32 epilogue tile would not fit 64 KiB well
        const long blocks = ((M + BP - 1) / BP) * ((d->cout + BM - 1) / BM);
        if (blocks >= (BP == 256 ? 1024 : 512) || i == 4) { bm = BM; bp = BP; break; }
    }
    out->bm = bm; out->bp = bp;
    out->depth = bp == 256 ? 3 : (steps <= 4 ? 2 : 4);
}

// Resolve the configuration of a launch the LDS-DMA path supports: the descriptor's explicit choice when given (validated), else the default.
static int ring_resolve(const lh_igemm_desc* d, int dtype, RingCfg* out) {
    if (d->cfg[0] == 0) {
        default_cfg(d, dtype, out);
        return LH_OK;
    }
    const RingCfg c = {d->cfg[0], d->cfg[1], d->cfg[2], d->cfg[3]};
    const LhConvKind kind = lh_conv_kind(c.depth);
    if (kind == LH_CONV_DIRECT && !d3_fits(d, dtype, c)) {
        lh_set_error("igemm: the direct 3x3 configuration (64, 256, 100, %d) does not fit this launch", c.kb);
        return LH_ERR_ARG;
    }
    if (kind == LH_CONV_POINTWISE && !pw_fits(d, dtype, c)) {
        lh_set_error("igemm: pointwise configuration panel %d x K %d, %d pixels per wave does not exist or does not fit this launch",
                     c.bm, c.kb, c.bp);
        return LH_ERR_ARG;
    }
    if (!lh_kind_persistent(kind) && !cfg_exists(dtype, c)) {         // (every code no kernel carries ends here)
        lh_set_error("igemm: configuration tile %dx%d depth %d kb %d is not compiled in for dtype %d", c.bm, c.bp, c.depth, c.kb, dtype);
        return LH_ERR_UNSUPPORTED;
    }
    // an explicit choice must pass the hard rules of the candidate list: weight packs are padded to 128 rows, so e.g. a
    // 256-row tile on a pack with an odd number of 128-row blocks would fetch past its end (the phases of a batched
    // launch share the lead's choice, so the soft rules -- tile wider than the problem, ring deeper than the loop -- stay legal)
    if (!lh_kind_persistent(kind) && !cfg_safe(d, dtype, c)) {
        lh_set_error("igemm: configuration tile %dx%d depth %d kb %d does not fit this launch (cout %d, k_run %d, %d taps)",
                     c.bm, c.bp, c.depth, c.kb, d->cout, d->k_run, d->ntaps);
        return LH_ERR_ARG;
    }
    *out = c;
    return LH_OK;
}

int lh_conv_plan(const lh_igemm_desc* d, int dtype, ConvPlan* out) {
    if (!lh_ring_supported(d, dtype)) {
        lh_staged_tile(d, dtype, &out->cfg);
    } else if (int rc = ring_resolve(d, dtype, &out->cfg)) {
        return rc;
    }
    out->kind = lh_conv_kind(out->cfg.depth);
    return LH_OK;
}

static void put_cfg(int* cfg5, const RingCfg& c) {
    cfg5[0] = c.bm; cfg5[1] = c.bp; cfg5[2] = c.depth; cfg5[3] = c.kb; cfg5[4] = 0;
}

static int ring_candidates(const lh_igemm_desc* d, int dtype, int* out, int max) {
    const RingCfg* t; int n, k = 0;
    cfg_table(dtype, &t, &n);
    for (int i = 0; i < n && k < max; ++i) {
        if (!cfg_fits(d, dtype, t[i])) continue;
        put_cfg(out + 5 * k++, t[i]);
    }
    if (k < max && d3_supported(d, dtype)) put_cfg(out + 5 * k++, {64, 256, LH_DIRECT_DEPTH, d->k_run});
    for (const PwCfg& c : kCfgPw) {
        const RingCfg r = {c.bm, 16 * c.pt, LH_POINTWISE_DEPTH, c.kc};
        if (k < max && pw_fits(d, dtype, r)) put_cfg(out + 5 * k++, r);
    }
    return k;
}


// rows of the slab a launch writes (statistics; gate_terms = 1 | 2: the partial sums of lh_igemm_gated): one per pixel tile, on the
// persistent kernels one per workgroup of a channel block -- the pointwise kernel's gate instantiations may hold a different number
// of workgroups per CU
static int rows(const lh_igemm_desc* d, const ConvPlan& p, int dtype, int gate_terms) {
    if (p.kind == LH_CONV_DIRECT) return d3_rows(d);
    if (p.kind == LH_CONV_POINTWISE) return pw_rows(d, p.cfg, dtype, gate_terms);
    return ceil_div((long)d->n * d->ho * d->wo, p.cfg.bp);
}

// the row queries cannot fail: an explicit cfg that does not resolve counts as cfg = 0
static int rows_or_default(const lh_igemm_desc* d, int dtype, int gate_terms) {
    ConvPlan p;
    if (lh_conv_plan(d, dtype, &p) != LH_OK) {
        default_cfg(d, dtype, &p.cfg);
        p.kind = lh_conv_kind(p.cfg.depth);
    }
    return rows(d, p, dtype, gate_terms);
}

extern "C" int lh_igemm_config(const lh_igemm_desc* d, int dtype, int* cfg5) {
    LH_REQUIRE(d && cfg5, "lh_igemm_config: null pointer");
    ConvPlan p;
    if (int rc = lh_conv_plan(d, dtype, &p)) return rc;
    put_cfg(cfg5, p.cfg);
    return LH_OK;
}

extern "C" int lh_igemm_tile(const lh_igemm_desc* d, int dtype, int* bm, int* bp, int* ring) {
    LH_REQUIRE(d && bm && bp && ring, "lh_igemm_tile: null pointer");
    ConvPlan p;
    if (int rc = lh_conv_plan(d, dtype, &p)) return rc;
    *bm = p.cfg.bm; *bp = p.cfg.bp;
    *ring = p.kind == LH_CONV_STAGED ? 0 : p.cfg.kb * 10 + p.cfg.depth;      // K bytes per stage * 10 + ring depth; 0 = register-staged kernel
    return LH_OK;
}

extern "C" int lh_igemm_candidates(const lh_igemm_desc* d, int dtype, int* cfgs, int max) {
    if (!d || !cfgs || max <= 0 || !lh_ring_supported(d, dtype)) return 0;
    return ring_candidates(d, dtype, cfgs, max);
}

extern "C" int lh_igemm_stats_rows(const lh_igemm_desc* d, int dtype) { return rows_or_default(d, dtype, 0); }

extern "C" int lh_igemm_gated_rows(const lh_igemm_desc* d, int dtype, int nterms) { return rows_or_default(d, dtype, nterms >= 2 ? 2 : 1); }

// ---- phase batching: 2..4 descriptors that differ only in taps / placement; the one with most taps leads (its cfg is the launch's)
int lh_phase_lead(const lh_igemm_desc* const* descs, int nphase) {
    int lead = 0;
    for (int i = 1; i < nphase; ++i)
        if (descs[i]->ntaps > descs[lead]->ntaps) lead = i;
    return lead;
}

bool lh_phases_ok(const lh_igemm_desc* const* descs, int nphase) {
    if (!descs || nphase < 2 || nphase > 4) return false;
    const lh_igemm_desc* a = descs[0];
    for (int i = 0; i < nphase; ++i) {
        const lh_igemm_desc* b = descs[i];
        if (!b || b->n != a->n || b->hi != a->hi || b->wi != a->wi || b->in_pix_stride != a->in_pix_stride || b->k_run != a->k_run ||
            b->ho != a->ho || b->wo != a->wo || b->sh != a->sh || b->sw != a->sw || b->cout != a->cout || b->OH != a->OH ||
            b->OW != a->OW || b->osh != a->osh || b->osw != a->osw || b->out_pix_stride != a->out_pix_stride || b->relu != a->relu)
            return false;
    }
    return true;
}

extern "C" int lh_igemm_phases_rows(const lh_igemm_desc* const* descs, int nphase, int dtype) {
    if (!lh_phases_ok(descs, nphase)) return -1;
    const lh_igemm_desc* d = descs[lh_phase_lead(descs, nphase)];
    return lh_ring_supported(d, dtype) ? rows_or_default(d, dtype, 0) : -1;
}
