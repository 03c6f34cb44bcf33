// Weight gradient, host side: the launch plan (tile, ring stage, ring depth, pixel splits), the argument block of a planned launch and
// the launchers of the LDS-DMA ring kernel that the instantiation units define.  Pure host arithmetic: nothing here touches the device.
#pragma once
#include "wgrad_ring_kernel.h"     // WgradArgs
#include "wgrad_cfgs.h"

// One launch plan: tile, pixel rows per ring stage (0 = register-staged kernel), ring depth, pixel splits, stages per split.
struct WgradPlan {
    int bo, bi, kps, depth, nsplit, sps;
};

// The LDS-DMA kernel for one element type (wgrad_ring_{bf16,f16}.hip, wgrad_table_{bf16,f16}.hip): one problem, up to LH_MULTI_MAX
// problems, a table of problems in device memory.  All return 1 when the configuration is not compiled in.
int lh_wgrad_ring_launch_bf16(const WgradArgs& a, const WgradPlan& c, hipStream_t s);
int lh_wgrad_ring_launch_f16(const WgradArgs& a, const WgradPlan& c, hipStream_t s);
int lh_wgrad_ring_multi_launch_bf16(const LhMulti<WgradArgs>& m, const WgradPlan& c, hipStream_t s);
int lh_wgrad_ring_multi_launch_f16(const LhMulti<WgradArgs>& m, const WgradPlan& c, hipStream_t s);
int lh_wgrad_ring_table_launch_bf16(const WgradArgs* tab, const int2* items, int n_items, int bo, int bi, int kps, int depth, hipStream_t s);
int lh_wgrad_ring_table_launch_f16(const WgradArgs* tab, const int2* items, int n_items, int bo, int bi, int kps, int depth, hipStream_t s);

// 16 zero bytes in device memory, the source of every masked LDS-DMA lane (wgrad.hip); null when the device cannot be asked.
const unsigned char* wgrad_zero_page();

struct WgradCfg { int bo, bi, depth, kps; };
static const WgradCfg kWCfg[] = {
#define X(BO, BI, WO, WI, D, KPS) {BO, BI, D, KPS},
    LH_WGRAD_CFGS(X)
#undef X
};
static const int kNWCfg = (int)(sizeof(kWCfg) / sizeof(WgradCfg));

static inline bool wgrad_cfg_compiled(int bo, int bi, int kps, int depth) {
    for (int i = 0; i < kNWCfg; ++i)
        if (kWCfg[i].bo == bo && kWCfg[i].bi == bi && kWCfg[i].depth == depth && kWCfg[i].kps == kps) return true;
    return false;
}

static inline bool wcfg_fits(const WgradCfg& c, int n_out, int n_in) {
    if (c.bo > 64 && n_out <= c.bo / 2) return false;
    if (c.bi > 64 && n_in <= c.bi / 2) return false;
    return true;
}

// The LDS-DMA kernel needs every x row it fetches 16-byte aligned: 16-byte pixel rows, or (NHWC4 stem: 8-byte pixels)
// an even horizontal stride, an aligned image pitch and tap column offsets that are multiples of two pixels.
static inline bool wgrad_ring_ok(const lh_igemm_desc* d, int es) {
    if (es != 2) return false;
    const long ps = (long)d->in_pix_stride * es;
    if (ps % 16 == 0) return true;
    if ((ps * d->sw) % 16 != 0 || (ps * d->wi) % 16 != 0) return false;
    for (int t = 0; t < d->ntaps; ++t)
        if ((ps * d->dw[t]) % 16 != 0) return false;
    return true;
}

// Pixel splits for a tile shape: `target` workgroups in all, at least `min_stages` ring stages per workgroup, at most
// ~24 MiB of fp32 slab (every split writes, and the fold re-reads, a full copy of the weight tensor).
static inline void wgrad_splits(const lh_igemm_desc* d, int n_out, int n_in, int bo, int bi, int kps, long target, int* nsplit, int* sps) {
    const long M = (long)d->n * d->ho * d->wo;
    const long stages = (M + kps - 1) / kps;
    const long tiles = (long)((n_out + bo - 1) / bo) * ((n_in + bi - 1) / bi) * d->ntaps;
    const long min_stages = 256 / kps;               // >= 256 pixels per workgroup
    long want = (target + tiles - 1) / tiles;
    long max_split = (stages + min_stages - 1) / min_stages;
    if (max_split > 128) max_split = 128;
    if (want > max_split) want = max_split;
    const long per_split_bytes = (long)n_out * n_in * d->ntaps * 4;
    long by_bytes = (24L << 20) / (per_split_bytes > 0 ? per_split_bytes : 1);
    if (by_bytes < 1) by_bytes = 1;
    if (want > by_bytes && tiles * by_bytes >= 256) want = by_bytes;
    if (want < 1) want = 1;
    *sps = (int)((stages + want - 1) / want);
    *nsplit = (int)((stages + *sps - 1) / *sps);
}

// Resolve the plan of a launch: the descriptor's explicit choice (cfg[5..7], validated) or the static default
// (tile by channel counts, 32-pixel stages, 4-stage ring, ~1024 workgroups).
static inline int wgrad_plan(const lh_igemm_desc* d, int n_out, int n_in, int dtype, WgradPlan* out) {
    const int es = lh_dtype_size(dtype);
    const bool ring = wgrad_ring_ok(d, es);
    const long M = (long)d->n * d->ho * d->wo;
    if (d->cfg[5] != 0) {
        const int enc = d->cfg[7];
        WgradPlan c = {d->cfg[5], d->cfg[6], (enc >> 16) & 0xff, (enc >> 24) & 0xff, enc & 0xffff, 0};
        if (!ring || !wgrad_cfg_compiled(c.bo, c.bi, c.kps, c.depth) || c.nsplit < 1) {
            lh_set_error("lh_wgrad: configuration tile %dx%d stage %d depth %d splits %d is not available for this launch", c.bo, c.bi, c.kps, c.depth, c.nsplit);
            return LH_ERR_UNSUPPORTED;
        }
        const WgradCfg wc = {c.bo, c.bi, c.depth, c.kps};
        if (!wcfg_fits(wc, n_out, n_in)) {          // same rule as lh_wgrad_candidates: an explicit choice must fit the gradient
            lh_set_error("lh_wgrad: tile %dx%d does not fit a %d x %d gradient", c.bo, c.bi, n_out, n_in);
            return LH_ERR_ARG;
        }
        const long stages = (M + c.kps - 1) / c.kps;
        c.sps = (int)((stages + c.nsplit - 1) / c.nsplit);
        c.nsplit = (int)((stages + c.sps - 1) / c.sps);
        *out = c;
        return LH_OK;
    }
    WgradPlan c;
    c.bo = n_out > 64 ? 128 : 64;
    c.bi = n_in > 64 ? 128 : 64;
    c.kps = ring ? 32 : 0;
    c.depth = ring ? 4 : 0;
    wgrad_splits(d, n_out, n_in, c.bo, c.bi, ring ? 32 : (dtype == LH_F32 ? 16 : 32), 1024, &c.nsplit, &c.sps);
    *out = c;
    return LH_OK;
}

// Check the arguments of one weight gradient and fill its argument block for plan `c` (fold_rows > 1: lh_wgrad_rowfold).  `zero` stays
// null: whoever launches the ring form sets it from wgrad_zero_page().
static inline int wgrad_fill_args(const lh_igemm_desc* d, const void* x, const void* dy, int dy_pix_stride, int n_out, int n_in, float* slab,
                                  int dtype, int fold_rows, const WgradPlan& c, WgradArgs* out) {
    LH_REQUIRE(d && x && dy && slab, "lh_wgrad: null pointer");
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0, "lh_wgrad: bad dtype %d", dtype);
    const int epc = 16 / es;
    LH_REQUIRE(d->ntaps > 0 && d->ntaps <= 64, "lh_wgrad: ntaps %d out of range", d->ntaps);
    LH_REQUIRE(n_in == d->k_run && n_in % epc == 0, "lh_wgrad: n_in %d must equal k_run %d and be a multiple of %d", n_in, d->k_run, epc);
    LH_REQUIRE(n_out % epc == 0 && dy_pix_stride % epc == 0 && dy_pix_stride >= n_out, "lh_wgrad: n_out %d / stride %d", n_out, dy_pix_stride);
    WgradArgs& a = *out;
    a.x = (const unsigned char*)x; a.dy = (const unsigned char*)dy; a.slab = slab; a.zero = nullptr;
    a.n = d->n; a.hi = d->hi; a.wi = d->wi; a.in_pix_stride = d->in_pix_stride; a.k_run = d->k_run;
    a.ho = d->ho; a.wo = d->wo; a.M = d->n * d->ho * d->wo; a.sh = d->sh; a.sw = d->sw;
    a.dy_pix_stride = dy_pix_stride; a.n_out = n_out; a.n_in = n_in; a.ntaps = d->ntaps;
    for (int i = 0; i < 64; ++i) { a.dh[i] = d->dh[i]; a.dw[i] = d->dw[i]; }
    a.fold_k = 0;
    a.nsplit = c.nsplit; a.steps_per_split = c.sps;
    a.i_tiles = ceil_div(n_in, c.bi);
    a.tiles = ceil_div(n_out, c.bo) * a.i_tiles;
    a.xcd = 1;
    a.adv_n = a.adv_a = a.adv_b = 0;
    if (fold_rows > 1) {
        LH_REQUIRE(c.kps && d->ntaps == 1 && n_in % fold_rows == 0 && (n_in / fold_rows) % epc == 0,
                   "lh_wgrad_rowfold: needs the LDS-DMA kernel, one tap and a run of whole 16-byte chunks per row");
        a.fold_k = n_in / fold_rows;
    }
    if (c.kps) {                  // LDS-DMA ring kernel: one stage of kps pixels as images + rows + columns
        const int hw = d->ho * d->wo;
        a.adv_n = c.kps / hw;
        a.adv_a = (c.kps % hw) / d->wo;
        a.adv_b = c.kps % d->wo;
    }
    return LH_OK;
}
