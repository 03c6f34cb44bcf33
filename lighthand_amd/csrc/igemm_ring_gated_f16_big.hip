// f16 instantiations of the gated LDS-DMA convolution kernel (igemm_ring_gated_kernel: the BatchNorm-backward gate in the epilogue),
// configuration part "big" (igemm_ring_inst.h).
#include "igemm_ring_cfgs.h"
#define LH_T f16
#define LH_FN lh_ring_gated_launch_f16_big
#define LH_LIST LH_RING_CFGS_BIG
#define LH_GATED
#include "igemm_ring_inst.h"
