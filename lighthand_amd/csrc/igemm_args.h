// Shared by the host layer of the forward / data-gradient convolution and its five kernels: the kernel-argument block (IgemmArgs), a
// kernel configuration (RingCfg) with the ONE rule that says which kernel a configuration runs on (lh_conv_kind), a resolved launch
// (ConvPlan), and what the layer's files offer each other:
//   igemm.hip         the launching entry points (lh_igemm, _gated, _multi, _phases, _phases_head): validate, fill, attach, launch
//   igemm_plan.hip    host arithmetic only: configuration tables, what fits a launch, default, resolve, candidates, slab rows, the queries
//   igemm_ring.hip    device pages and the dispatch into the per-type instantiation files of the LDS-DMA, pointwise and direct kernels
//   igemm_staged.hip  the register-staged fallback kernel (igemm_staged_kernel.h), its tile choice and launch
#pragma once
#include "common.h"
#include "igemm_ring_cfgs.h"

struct IgemmArgs {
    const unsigned char* in;
    const unsigned char* w;
    unsigned char* out;
    const unsigned char* addend;
    const unsigned char* addend_mask; // optional: ReLU mask bits (lh_fuse_fwd relu_mask) gating the addend element-wise
    const unsigned char* zero;       // 16 zero bytes in device memory (LDS-DMA kernel: what masked lanes fetch)
    unsigned char* dump;             // 1 KiB nobody reads: where the persistent kernels' masked lanes STORE (fixed store count per tile)
    const float* bias;
    const float* scale;      // optional per-output-channel affine applied to the fp32 accumulator (eval-mode BN fold)
    const float* shift;
    float* stats;
    // BatchNorm-backward gate (lh_igemm_gated): the launch's output is the gradient of relu(BN(gx)); the epilogue stores the
    // gated gradient and `stats` receives { sum g, sum g * xhat } instead of { sum v, sum v^2 }
    const unsigned char* gx;
    const float* gmean;
    const float* ginv;
    const float* gscale;
    const float* gshift;
    const unsigned char* gmask;      // optional: the activation is a residual tail relu(BN(gx) + r) -- its sign comes from the stored mask bits
    const unsigned char* gx2;        // optional (with gmask, pointwise kernel): r = BN2(gx2), a projection shortcut -- `stats2` takes { sum g, sum g * xhat2 }
    const float* gmean2;
    const float* ginv2;
    float* stats2;
    // Fused 1x1 head (lh_igemm_phases_head, 256 x 256 tile only): the tile -- after affine + ReLU -- is multiplied by
    // head_w [>= 32 rows][cout] (K-major pack rows of the 1x1 convolution, rows >= head_j zero) inside the epilogue and
    // only head_out[n][j][OH][OW] (fp32) is written; `out` is not touched
    const unsigned char* head_w;
    const float* head_bias;
    float* head_out;
    int head_j, head_wstride;       // valid head channels (<= 32), bytes between head_w rows
    int n, hi, wi, in_pix_stride, k_run, kspt, kpad;   // kpad: elements per (row, tap) of the weight pack
    int ho, wo, M, sh, sw, cout;
    int OH, OW, osh, osw, ooh, oow, out_pix_stride;
    int ntaps, relu;
    // Phase batching (lh_igemm_phases): up to 4 launches that differ only in weight pack, tap grid, output placement and
    // stats rows (the sub-pixel phases of stride-2 transposed forms) run as ONE grid of nphase * phase_blocks work items.
    int nphase, phase_blocks;
    const unsigned char* ph_w[4];
    int ph_ntaps[4], ph_tw[4], ph_dh0[4], ph_dhs[4], ph_dw0[4], ph_dws[4], ph_ooh[4], ph_oow[4], ph_row0[4];
    int xcd;                         // ring kernel: XCD-aware work-item order (always on: speed only)
    int pw_g, pw_cb;                 // pointwise kernel (igemm_pw_kernel.h): workgroups per channel block, channel blocks
    int tw, dh0, dhs, dw0, dws;      // regular tap grid (ring kernel): tap t = (t / tw, t % tw)
    signed char dh[64];
    signed char dw[64];
};

// One kernel configuration = lh_igemm_desc.cfg[0..3].  `depth` names the kernel (lh_conv_kind):
//   0        register-staged fallback (igemm_staged_kernel.h): bm x bp tile, kb = 0
//   1        persistent pointwise kernel (igemm_pw_kernel.h): bm = channels of the resident weight panel, bp = pixels a wave takes per
//            step (16 * PT), kb = padded K of the panel in elements
//   2..9     LDS-DMA kernel (igemm_ring_kernel.h): tile (output channels x pixels), ring depth, kb = K bytes per stage
//   20..29   its dense-wave forms: ring depth + LH_DENSE_DEPTH (igemm_ring_cfgs.h)
//   100      direct 3x3 kernel (conv3x3_direct_kernel.h): bm = 64, bp = 256 (a 16 x 16 output tile), kb = input channels per tap (32 | 64)
// No kernel carries another code: lh_igemm_config refuses it.
struct RingCfg {
    int bm, bp, depth, kb;
};

enum LhConvKind { LH_CONV_NONE, LH_CONV_STAGED, LH_CONV_POINTWISE, LH_CONV_TILED, LH_CONV_DENSE, LH_CONV_DIRECT };
enum { LH_POINTWISE_DEPTH = 1, LH_DIRECT_DEPTH = 100 };

static inline LhConvKind lh_conv_kind(int depth) {
    return depth == 0 ? LH_CONV_STAGED : depth == LH_POINTWISE_DEPTH ? LH_CONV_POINTWISE : depth >= 2 && depth < 10 ? LH_CONV_TILED
         : depth >= LH_DENSE_DEPTH && depth < LH_DENSE_DEPTH + 10 ? LH_CONV_DENSE : depth == LH_DIRECT_DEPTH ? LH_CONV_DIRECT : LH_CONV_NONE;
}
// ring depth of a tiled or dense-wave configuration
static inline int lh_ring_depth(const RingCfg& c) { return lh_conv_kind(c.depth) == LH_CONV_DENSE ? c.depth - LH_DENSE_DEPTH : c.depth; }
// pointwise and direct: one workgroup walks many tiles (single launches only; statistics rows per workgroup, not per pixel tile)
static inline bool lh_kind_persistent(LhConvKind k) { return k == LH_CONV_POINTWISE || k == LH_CONV_DIRECT; }
// kernels with a BatchNorm-backward gate (lh_igemm_gated, 16-bit types), and the one that gates two BatchNorm terms
static inline bool lh_kind_gated(LhConvKind k) { return k != LH_CONV_STAGED && k != LH_CONV_NONE; }
static inline bool lh_kind_gates_two(LhConvKind k) { return k == LH_CONV_POINTWISE; }

// A resolved launch: the kernel and its configuration (lh_conv_plan)
struct ConvPlan {
    LhConvKind kind;
    RingCfg cfg;
};

// workgroups per channel block of a pointwise launch: every CU holds `occ` workgroups for the whole launch (occ = what the
// occupancy query reports for the instantiation, 1..4: lh_pw_occupancy)
static inline int lh_pw_lds_bytes(int bm, int kc, int pt, int gate = 0) {      // panel, staging, per-channel constants (2 vectors; 4 / 6 with the gate of one / two BatchNorm terms)
    return bm * kc * 2 + 4 * pt * 16 * (64 * 2 + 8) + (2 + 2 * gate) * bm * 4;
}

static inline void lh_pw_grid(int bm, int kc, int pt, long M, int cout, int occ, int* G, int* CB) {
    const int cb = (cout + bm - 1) / bm;
    const long ntile = (M + pt * 16 - 1) / (pt * 16);
    long g = 256L * occ / cb / 8 * 8;
    const long need = ((ntile + 3) / 4 + 7) / 8 * 8;           // no more workgroups than there are wave tiles
    if (g > need) g = need;
    if (g < 8) g = 8;
    *G = (int)g;
    *CB = cb;
}


// igemm_plan.hip
bool lh_tap_grid(const lh_igemm_desc* d, int* tw, int* dh0, int* dhs, int* dw0, int* dws);
bool lh_ring_supported(const lh_igemm_desc* d, int dtype);
int lh_conv_plan(const lh_igemm_desc* d, int dtype, ConvPlan* out);     // supported -> resolve (explicit cfg validated, else the default); else the staged tile
int lh_pw_occupancy(const RingCfg& c, int dtype, int mode);      // mode: 0 plain, 1 statistics, 2 / 3 BatchNorm-backward gate of one / two terms
bool lh_phases_ok(const lh_igemm_desc* const* descs, int nphase);
int lh_phase_lead(const lh_igemm_desc* const* descs, int nphase);
// igemm_staged.hip
void lh_staged_tile(const lh_igemm_desc* d, int dtype, RingCfg* out);
int lh_staged_launch(const IgemmArgs& a, const RingCfg& c, int dtype, hipStream_t s);
// igemm_ring.hip
int lh_conv_launch(const IgemmArgs& a, const ConvPlan& p, int dtype, hipStream_t s);
template <typename A> struct LhMulti;
int lh_igemm_ring_multi_launch(LhMulti<IgemmArgs>& m, const RingCfg& c, int dtype, hipStream_t s);
