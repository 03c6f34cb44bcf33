// The fused "sum of affine terms (+ nearest upsample) + ReLU" elementwise op, forward: one call, or the same layer position
// of several independent calls as one multi-problem launch.
#include "bn_common.h"
#include "multi.h"
#include <type_traits>
#include <vector>

struct FuseArgs {
    int exp;                     // bn_exp_flags() >> 2 (forward bits)
    const unsigned char* x[4];
    const float* scale[4];
    const float* shift[4];
    int log2up[4];
    int nterms, relu;
    unsigned char* out;
    unsigned char* mask;         // optional: one byte per 16-byte chunk of `out`, bit e = (element e > 0)
    int n, h, w, c;
    long total;                  // 16-byte chunks of `out` (flat kernels)
    const unsigned char* touch;  // optional (lh_fuse_desc.l2_touch): bytes the NEXT launch on the stream will read first -- its weight pack
    unsigned touch_bytes;
};

template <typename T> struct fuse_fwd {
using Args = FuseArgs;
static __device__ __forceinline__ void run(const FuseArgs& p, const int bid, const int nblk) {
    constexpr int EPC = 16 / sizeof(T);
    const int nchunk = p.c / EPC;
    const long total = (long)p.n * p.h * p.w * nchunk;
    for (long idx = (long)bid * 256 + threadIdx.x; idx < total; idx += (long)nblk * 256) {
        // 32-bit index arithmetic (plan_fuse_fwd checks total < 2^31): 64-bit divisions cost more than the rest of the loop
        const unsigned iu = (unsigned)idx;
        const unsigned pix = iu / (unsigned)nchunk;
        const int ch = (int)(iu - pix * (unsigned)nchunk);
        const unsigned t2 = pix / (unsigned)p.w;
        const int x = (int)(pix - t2 * (unsigned)p.w);
        const int n = (int)(t2 / (unsigned)p.h), y = (int)(t2 - (unsigned)n * (unsigned)p.h);
        float acc[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
        for (int t = 0; t < p.nterms; ++t) {
            const int l = p.log2up[t];
            const long sp = ((long)n * (p.h >> l) + (y >> l)) * (p.w >> l) + (x >> l);
            float v[EPC];
            unpack16<T>(*reinterpret_cast<const uint4*>(p.x[t] + (sp * p.c + ch * EPC) * sizeof(T)), v);
            if (p.scale[t]) {
                const float* sc = p.scale[t] + ch * EPC;
                const float* sh = p.shift[t] + ch * EPC;
#pragma unroll
                for (int e = 0; e < EPC; ++e) v[e] = v[e] * sc[e] + sh[e];
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] += v[e];
        }
        if (p.relu) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = fmaxf(acc[e], 0.f);
        }
        const uint4 u = pack16<T>(acc);
        *reinterpret_cast<uint4*>(p.out + idx * 16) = u;
        if (p.mask) p.mask[idx] = positive_bits<T>(u);
    }
}
};

// Fast path: no upsampled term, <= 2 terms, channel chunks a power of two <= 256.  The grid stride is a multiple of
// the chunk count, so a thread keeps ONE channel chunk: its scale/shift live in registers and the loop has no
// integer division -- the kernel is a pure 16-byte-per-lane stream.
template <typename T, int NT> struct fuse_fwd_flat {
using Args = FuseArgs;
static __device__ __forceinline__ void run(const FuseArgs& p, const int bid, const int nblk) {
    const long total = p.total;
    constexpr int EPC = 16 / sizeof(T);
    const int nchunk = p.c / EPC;
    const int ch = threadIdx.x & (nchunk - 1);
    float sc[NT][EPC], sh[NT][EPC];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (p.scale[t]) { load_vec<EPC>(p.scale[t] + ch * EPC, sc[t]); load_vec<EPC>(p.shift[t] + ch * EPC, sh[t]); }
        else { fill_vec<EPC>(sc[t], 1.f); fill_vec<EPC>(sh[t], 0.f); }
    }
    const long stride = (long)nblk * 256;
    const long rounds = (total + stride - 1) / stride;
    const bool rev = p.exp & 2;
    auto body = [&](auto NTc) __attribute__((always_inline)) {
    constexpr bool LNT = decltype(NTc)::value;
    for (long rr = 0; rr < rounds; ++rr) {
        const long idx = walk_round(rr, rounds, rev) * stride + (long)bid * 256 + threadIdx.x;
        if (idx >= total) continue;
        float acc[EPC];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float v[EPC];
            unpack16<T>(ld16<LNT>(p.x[t] + idx * 16), v);
            if (p.scale[t]) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) v[e] = v[e] * sc[t][e] + sh[t][e];
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = t == 0 ? v[e] : acc[e] + v[e];
        }
        if (p.relu) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = fmaxf(acc[e], 0.f);
        }
        const uint4 u = pack16<T>(acc);
        *reinterpret_cast<uint4*>(p.out + idx * 16) = u;
        if (p.mask) p.mask[idx] = positive_bits<T>(u);
    }
    };
    if (p.exp & 1) body(std::true_type{}); else body(std::false_type{});
    lh_l2_touch(p.touch, p.touch_bytes, bid, nblk);
}
};

// (Round 4's channel-slice form -- BatchNorm finalize + apply as ONE launch for small tensors -- was measured slower than the two launches
//  (the fold every workgroup repeats costs more than the 5.4 us finalize launch it removes) and removed in round 6.)

// ---- launch records: a C-ABI call is first PLANNED into the kernel launches it consists of (kind, grid, argument block),
// then run -- one record as a plain launch, the records of several independent calls that agree in kind as one
// multi-problem launch (multi.h).
enum FwdKind { K_FF_GEN, K_FF_FLAT1, K_FF_FLAT2 };
struct FwdLaunch {
    int kind, grid;
    FuseArgs a;
};

// pre_fin (out): bit t set when term t carries a BatchNorm finalize (lh_fuse_desc.fin) that has not run yet: the caller
// launches it first (no kernel of this file folds statistics).
static int plan_fuse_fwd(const lh_fuse_desc* d, void* out, int n, int h, int w, int c, int dtype, FwdLaunch& r, int& pre_fin) {
    LH_REQUIRE(d && out && d->nterms >= 1 && d->nterms <= 4, "lh_fuse_fwd: bad descriptor");
    const int es = lh_dtype_size(dtype);
    LH_REQUIRE(es > 0 && c % (16 / es) == 0, "lh_fuse_fwd: c %d not a multiple of the 16-byte chunk", c);
    FuseArgs& a = r.a;
    for (int t = 0; t < 4; ++t) {
        a.x[t] = t < d->nterms ? (const unsigned char*)d->x[t] : nullptr;
        a.scale[t] = t < d->nterms ? d->scale[t] : nullptr;
        a.shift[t] = t < d->nterms ? d->shift[t] : nullptr;
        a.log2up[t] = t < d->nterms ? d->log2up[t] : 0;
        if (t < d->nterms) {
            LH_REQUIRE(a.x[t], "lh_fuse_fwd: term %d has no input", t);
            LH_REQUIRE(a.log2up[t] >= 0 && (h >> a.log2up[t]) << a.log2up[t] == h && (w >> a.log2up[t]) << a.log2up[t] == w,
                       "lh_fuse_fwd: %dx%d not divisible by 2^%d", h, w, a.log2up[t]);
            LH_REQUIRE((a.scale[t] == nullptr) == (a.shift[t] == nullptr), "lh_fuse_fwd: scale/shift must come together");
        }
    }
    a.nterms = d->nterms; a.relu = d->relu; a.out = (unsigned char*)out; a.mask = (unsigned char*)d->relu_mask; a.n = n; a.h = h; a.w = w; a.c = c;
    const int nchunk = c / (16 / es);
    const long total = (long)n * h * w * nchunk;
    LH_REQUIRE(total < (1L << 31), "lh_fuse_fwd: tensor too large for 32-bit chunk indices");
    a.total = total;
    a.exp = bn_exp_flags() >> 2;
    a.touch_bytes = lh_touch_bytes(d->l2_touch, d->l2_touch_bytes);
    a.touch = a.touch_bytes ? (const unsigned char*)d->l2_touch : nullptr;
    bool flat = d->nterms <= 2 && bn_flat_chunks(nchunk);
    for (int t = 0; t < d->nterms; ++t) flat = flat && a.log2up[t] == 0;
    pre_fin = 0;
    for (int t = 0; t < d->nterms; ++t) {
        const lh_bn_finalize_call* f = d->fin[t];
        if (!f) continue;
        LH_REQUIRE(f->stats && f->rows > 0 && f->count > 0 && f->c == c && f->scale == d->scale[t] && f->shift == d->shift[t] && f->scale && f->shift,
                   "lh_fuse_fwd: term %d: the pending finalize must produce this term's scale / shift (c %d vs %d)", t, f->c, c);
        pre_fin |= 1 << t;
    }
    if (flat) {
        r.grid = flat_grid(total);      // >= 4 chunks per thread
        r.kind = d->nterms == 1 ? K_FF_FLAT1 : K_FF_FLAT2;
    } else {
        r.grid = generic_grid(total);
        r.kind = K_FF_GEN;
    }
    return LH_OK;
}

// Run n <= LH_MULTI_MAX records of ONE kind: a plain launch for one, a multi-problem launch for several.
static int bn_run(const FwdLaunch* const* L, int n, int dtype, hipStream_t s) {
    LH_REQUIRE(n >= 1 && n <= LH_MULTI_MAX, "bn_run: %d records", n);
    switch (L[0]->kind) {
        case K_FF_GEN: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_fwd<T>>(L, n, &FwdLaunch::a, s)); break;
        case K_FF_FLAT1: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_fwd_flat<T, 1>>(L, n, &FwdLaunch::a, s)); break;
        case K_FF_FLAT2: LH_DISPATCH_DTYPE(dtype, T, lh_launch_records<fuse_fwd_flat<T, 2>>(L, n, &FwdLaunch::a, s)); break;
        default: lh_set_error("bn_run: unknown kind %d", L[0]->kind); return LH_ERR_ARG;
    }
    LH_LAUNCH_CHECK("BatchNorm / ReLU pass launch");
    return LH_OK;
}

extern "C" int lh_fuse_fwd(const lh_fuse_desc* d, void* out, int n, int h, int w, int c, int dtype, void* stream) {
    FwdLaunch r;
    int pre = 0;
    int rc = plan_fuse_fwd(d, out, n, h, w, c, dtype, r, pre);
    if (rc) return rc;
    lh_bn_finalize_call fins[4];                  // at most one pending finalize per term: no heap allocation on the launch path
    int nf = 0;
    for (int t = 0; t < d->nterms && t < 4; ++t)
        if ((pre >> t) & 1) fins[nf++] = *d->fin[t];
    if (nf) rc = lh_bn_finalize_multi(fins, nf, stream);
    if (rc) return rc;
    const FwdLaunch* L[1] = {&r};
    return bn_run(L, 1, dtype, (hipStream_t)stream);
}

// the published kind values (include/lighthand_hip.h) are the planner's
static_assert(LH_FF_GEN == K_FF_GEN, "LH_FF_GEN");
static_assert(LH_FF_FLAT1 == K_FF_FLAT1, "LH_FF_FLAT1");
static_assert(LH_FF_FLAT2 == K_FF_FLAT2, "LH_FF_FLAT2");

// The kernel lh_fuse_fwd would launch for these arguments and its grid; nothing is launched (host arithmetic only).
extern "C" int lh_fuse_fwd_plan(const lh_fuse_desc* d, void* out, int n, int h, int w, int c, int dtype, int* kind, int* grid) {
    FwdLaunch r;
    int pre = 0;
    const int rc = plan_fuse_fwd(d, out, n, h, w, c, dtype, r, pre);
    if (rc) return rc;
    if (kind) *kind = r.kind;
    if (grid) *grid = r.grid;
    return LH_OK;
}

// n independent calls: their pending finalizes first, as one multi-problem launch; then the calls LH_MULTI_MAX per launch
// when all of them planned the same kind (the parallel branches of an HRNet module do), else one by one.
extern "C" int lh_fuse_fwd_multi(const lh_fuse_fwd_call* calls, int n, int dtype, void* stream) {
    LH_REQUIRE(calls && n >= 1, "lh_fuse_fwd_multi: bad arguments");
    std::vector<FwdLaunch> plans(n);
    std::vector<lh_bn_finalize_call> fins;
    bool same = true;
    for (int i = 0; i < n; ++i) {
        int pre = 0;
        const int rc = plan_fuse_fwd(calls[i].d, calls[i].out, calls[i].n, calls[i].h, calls[i].w, calls[i].c, dtype, plans[i], pre);
        if (rc) return rc;
        for (int t = 0; t < calls[i].d->nterms; ++t)
            if ((pre >> t) & 1) fins.push_back(*calls[i].d->fin[t]);
        same = same && plans[i].kind == plans[0].kind;
    }
    if (!fins.empty()) {
        const int rc = lh_bn_finalize_multi(fins.data(), (int)fins.size(), stream);
        if (rc) return rc;
    }
    const int per = same ? LH_MULTI_MAX : 1;
    for (int i0 = 0; i0 < n; i0 += per) {
        const FwdLaunch* L[LH_MULTI_MAX];
        const int m = n - i0 < per ? n - i0 : per;
        for (int i = 0; i < m; ++i) L[i] = &plans[i0 + i];
        const int rc = bn_run(L, m, dtype, (hipStream_t)stream);
        if (rc) return rc;
    }
    return LH_OK;
}
