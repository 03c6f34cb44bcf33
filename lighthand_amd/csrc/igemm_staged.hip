// Host side of the register-staged fallback kernel (igemm_staged_kernel.h): its tile choice and its launch.
#include "igemm_staged_kernel.h"

// 128 rows for more than 64 output channels; 128 pixels where that still gives >= 384 workgroups
void lh_staged_tile(const lh_igemm_desc* d, int dtype, RingCfg* out) {
    const long M = (long)d->n * d->ho * d->wo;
    int BM = d->cout > 64 ? 128 : 64;
    int BP = 128;
    if (dtype == LH_F32 && BM == 128) BP = 64;          // LDS budget of the fp32 epilogue tile
    const long blocks = ((M + BP - 1) / BP) * ((d->cout + BM - 1) / BM);
    if (BP == 128 && blocks < 384) BP = 64;
    *out = {BM, BP, 0, 0};
}

int lh_staged_launch(const IgemmArgs& a, const RingCfg& c, int dtype, hipStream_t s) {
    const int bm = c.bm, bp = c.bp;
#define LH_TILE(T)                                                               \
    if (bm == 128 && bp == 128) return launch_tile<T, 128, 128, 2, 2>(a, s);     \
    if (bm == 128 && bp == 64) return launch_tile<T, 128, 64, 4, 1>(a, s);       \
    if (bm == 64 && bp == 128) return launch_tile<T, 64, 128, 1, 4>(a, s);       \
    return launch_tile<T, 64, 64, 2, 2>(a, s);
    switch (dtype) {
        case LH_BF16: { LH_TILE(bf16) }
        case LH_F16: { LH_TILE(f16) }
        case LH_F32: {
            if (bm == 128) return launch_tile<float, 128, 64, 4, 1>(a, s);
            if (bp == 128) return launch_tile<float, 64, 128, 1, 4>(a, s);
            return launch_tile<float, 64, 64, 2, 2>(a, s);
        }
    }
#undef LH_TILE
    lh_set_error("lh_igemm: unsupported dtype %d", dtype);
    return LH_ERR_ARG;
}
