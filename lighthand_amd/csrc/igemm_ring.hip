// Launch side of the LDS-DMA convolution kernel (igemm_ring_kernel.h) and of the two persistent kernels (igemm_pw_kernel.h,
// conv3x3_direct_kernel.h): the device pages their masked lanes use, the 2 GiB reach check, and the dispatch of a resolved launch
// (ConvPlan, igemm_plan.hip) into the per-type instantiation files.
#include "common.h"

#include "igemm_args.h"
#include "multi.h"
#include <cstdlib>
#include <mutex>

// The tiled kernels are instantiated in four parts per element type, plain and gated (igemm_ring_gated_kernel: launches that carry a
// BatchNorm-backward gate), each a translation unit of its own whose launcher answers 1 for a configuration of another part.
typedef int (*RingLaunch)(const IgemmArgs& a, const RingCfg& c, hipStream_t s);
#define LH_RING_PARTS(X, PREFIX) X(PREFIX##big) X(PREFIX##mid) X(PREFIX##small) X(PREFIX##dense)
#define LH_DECLARE(F) int F(const IgemmArgs& a, const RingCfg& c, hipStream_t s);
#define LH_ENTRY(F) F,
LH_RING_PARTS(LH_DECLARE, lh_ring_launch_bf16_)
LH_RING_PARTS(LH_DECLARE, lh_ring_gated_launch_bf16_)
LH_RING_PARTS(LH_DECLARE, lh_ring_launch_f16_)
LH_RING_PARTS(LH_DECLARE, lh_ring_gated_launch_f16_)
static const RingLaunch kRingParts[2][2][4] = {       // [bf16 | f16][plain | gated][part]
    {{LH_RING_PARTS(LH_ENTRY, lh_ring_launch_bf16_)}, {LH_RING_PARTS(LH_ENTRY, lh_ring_gated_launch_bf16_)}},
    {{LH_RING_PARTS(LH_ENTRY, lh_ring_launch_f16_)}, {LH_RING_PARTS(LH_ENTRY, lh_ring_gated_launch_f16_)}}};
LH_DECLARE(lh_ring_launch_f32)
LH_DECLARE(lh_pw_launch_bf16)
LH_DECLARE(lh_pw_launch_f16)
LH_DECLARE(lh_d3_launch_bf16)
LH_DECLARE(lh_d3_launch_f16)
#undef LH_ENTRY
#undef LH_DECLARE
int lh_ring_multi_launch_bf16(const LhMulti<IgemmArgs>& m, const RingCfg& c, hipStream_t s);
int lh_ring_multi_launch_f16(const LhMulti<IgemmArgs>& m, const RingCfg& c, hipStream_t s);

// 16 zero bytes in device memory: the source of every LDS-DMA lane that falls outside the image or the K run.
// One copy per device (module memory); its address is looked up once per device.
__device__ __attribute__((aligned(16))) unsigned int lh_zero_page[4] = {0u, 0u, 0u, 0u};

// 1 KiB that is only ever written: the persistent kernels store the lanes that fall outside the problem here instead of
// predicating the store away, so every tile issues the same number of store instructions and the counted waits
// (s_waitcnt vmcnt) that keep a tile's stores in flight across the next tile stay exact.
__device__ __attribute__((aligned(16))) unsigned int lh_dump_page[256];

// address of one of this module's device arrays on the current device, looked up once per device
template <typename S>
static unsigned char* page_address(const S& symbol, unsigned char** cache) {
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!cache[dev]) {
        void* q = nullptr;
        if (hipGetSymbolAddress(&q, symbol) != hipSuccess) return nullptr;
        cache[dev] = (unsigned char*)q;
    }
    return cache[dev];
}

const unsigned char* lh_ring_zero_page() {                             // (bottleneck_infer.hip as well)
    static unsigned char* ptr[64] = {nullptr};
    return page_address(HIP_SYMBOL(lh_zero_page), ptr);
}
unsigned char* lh_ring_dump_page() {
    static unsigned char* ptr[64] = {nullptr};
    return page_address(HIP_SYMBOL(lh_dump_page), ptr);
}

// The buffer form of the tiled kernel's operand path (igemm_ring_kernel.h) addresses a tile's pixels with 32-bit offsets
// relative to the first image the tile touches, and marks masked lanes with offset 2^31: everything a tile can reach --
// the images a tile of `bp` pixels spans, the tap window in front of them, a weight block -- must stay below 2^31 bytes.
static int lh_ring_offsets_fit(const IgemmArgs& a, int bm, int bp, int es) {
    const long ipix = (long)a.in_pix_stride * es, img = (long)a.hi * a.wi * ipix;
    const long hw = (long)a.ho * a.wo > 0 ? (long)a.ho * a.wo : 1;
    long reach = (bp / hw + 2) * img;
    for (int ph = 0; ph < (a.nphase > 1 ? a.nphase : 1); ++ph) {
        const int ntaps = a.nphase > 1 ? a.ph_ntaps[ph] : a.ntaps, tw = a.nphase > 1 ? a.ph_tw[ph] : a.tw;
        const int dh0 = a.nphase > 1 ? a.ph_dh0[ph] : a.dh0, dhs = a.nphase > 1 ? a.ph_dhs[ph] : a.dhs;
        const int dw0 = a.nphase > 1 ? a.ph_dw0[ph] : a.dw0, dws = a.nphase > 1 ? a.ph_dws[ph] : a.dws;
        const int th = tw > 0 ? (ntaps + tw - 1) / tw : 1;
        const long shift = ((long)(std::abs(dh0) + std::abs(dhs) * th) * a.wi + std::abs(dw0) + std::abs(dws) * tw) * ipix;
        LH_REQUIRE(reach + 2 * shift + (long)a.k_run * es + 256 < (1L << 31) && (long)bm * ntaps * a.kpad * es < (1L << 31),
                   "igemm_ring: a %d-pixel tile of this launch reaches %ld bytes of input (%d x %d pixels of %ld bytes per image, tap window %ld) "
                   "or %ld bytes of weights: more than the 2 GiB a workgroup's buffer descriptor addresses",
                   bp, reach + 2 * shift, a.hi, a.wi, ipix, shift, (long)bm * ntaps * a.kpad * es);
    }
    return LH_OK;
}

// Launch a resolved problem on the kernel its plan names.
int lh_conv_launch(const IgemmArgs& a0, const ConvPlan& p, int dtype, hipStream_t s) {
    const RingCfg& c = p.cfg;
    if (p.kind == LH_CONV_STAGED) return lh_staged_launch(a0, c, dtype, s);
    IgemmArgs a = a0;
    a.zero = lh_ring_zero_page();
    a.dump = lh_ring_dump_page();
    if (!a.zero || !a.dump) {
        lh_set_error("igemm_ring: cannot resolve the zero page on this device");
        return LH_ERR_HIP;
    }
    const int f16 = dtype == LH_F16, bits16 = f16 || dtype == LH_BF16;
    int rc = 1;
    if (p.kind == LH_CONV_DIRECT) {
        if (bits16) rc = (f16 ? lh_d3_launch_f16 : lh_d3_launch_bf16)(a, c, s);
        if (rc == 1) {
            lh_set_error("conv3x3_direct: no kernel for %d input channels, dtype %d", c.kb, dtype);
            return LH_ERR_UNSUPPORTED;
        }
        return rc;
    }
    if (p.kind == LH_CONV_POINTWISE) {
        if (bits16) rc = (f16 ? lh_pw_launch_f16 : lh_pw_launch_bf16)(a, c, s);
        if (rc == 1) {
            lh_set_error("igemm_pw: no kernel for panel %d x K %d, %d pixels per wave, dtype %d", c.bm, c.kb, c.bp, dtype);
            return LH_ERR_UNSUPPORTED;
        }
        return rc;
    }
    if (int e = lh_ring_offsets_fit(a, c.bm, c.bp, dtype == LH_F32 ? 4 : 2)) return e;
    const bool gated = a.gx != nullptr;                  // the gate is compiled into kernels of its own (igemm_ring_gated_kernel)
    if (bits16) {
        for (RingLaunch part : kRingParts[f16][gated])
            if ((rc = part(a, c, s)) != 1) break;
    } else if (dtype != LH_F32) {
        lh_set_error("igemm_ring: unsupported dtype %d", dtype);
        return LH_ERR_ARG;
    } else if (gated) {
        lh_set_error("igemm_ring: the BatchNorm-backward gate exists for the 16-bit types only");
        return LH_ERR_UNSUPPORTED;
    } else {
        rc = lh_ring_launch_f32(a, c, s);
    }
    if (rc == 1) {
        lh_set_error("igemm_ring: no kernel for tile %dx%d depth %d kb %d dtype %d", c.bm, c.bp, c.depth, c.kb, dtype);
        return LH_ERR_UNSUPPORTED;
    }
    return rc;
}

int lh_igemm_ring_multi_launch(LhMulti<IgemmArgs>& m, const RingCfg& c, int dtype, hipStream_t s) {
    const unsigned char* z = lh_ring_zero_page();
    if (!z) {
        lh_set_error("igemm_ring_multi: cannot resolve the zero page on this device");
        return LH_ERR_HIP;
    }
    for (int i = 0; i < m.n; ++i) { m.a[i].zero = z; m.a[i].dump = lh_ring_dump_page(); }
    for (int i = 0; i < m.n; ++i)                        // (lh_igemm_multi has no gate argument; the multi-problem kernel is compiled without one)
        LH_REQUIRE(!m.a[i].gx, "igemm_ring_multi: problem %d carries a BatchNorm-backward gate, which the multi-problem kernel does not have", i);
    for (int i = 0; i < m.n; ++i)
        if (int e = lh_ring_offsets_fit(m.a[i], c.bm, c.bp, 2)) return e;
    int rc = 1;
    if (dtype == LH_BF16) rc = lh_ring_multi_launch_bf16(m, c, s);
    else if (dtype == LH_F16) rc = lh_ring_multi_launch_f16(m, c, s);
    if (rc == 1) {
        lh_set_error("igemm_ring_multi: no multi-problem kernel for tile %dx%d depth %d kb %d dtype %d (4-wave tiles, 16-bit types)",
                     c.bm, c.bp, c.depth, c.kb, dtype);
        return LH_ERR_UNSUPPORTED;
    }
    return rc;
}
