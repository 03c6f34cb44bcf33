// fp16 instantiations of the single- and multi-problem forms of the LDS-DMA weight-gradient kernel (wgrad_ring_inst.h).
#include "wgrad_ring_inst.h"
LH_WGRAD_RING_LAUNCHERS(lh_wgrad_ring_launch_f16, lh_wgrad_ring_multi_launch_f16, f16)
