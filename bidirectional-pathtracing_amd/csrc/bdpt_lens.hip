// bdpt_lens.hip — the thin-lens flavour (EXT = 3) of k_bdpt_sample: its explicit
// instantiations for every MAXV class, STATS value and LDS mode, in a translation unit of their own
// so that they compile beside bdpt_hip.hip, which launches them (launch_maxv).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see __graft_entry__.build).

#include "bdpt_megakernel.h"

namespace bdpt {

#define BDPT_LENS_KERNEL_DEF(MAXV, STATS, LM) template __global__ void k_bdpt_sample<MAXV, STATS, LM, 3>(KParams);
BDPT_LENS_KERNELS(BDPT_LENS_KERNEL_DEF)
#undef BDPT_LENS_KERNEL_DEF

}  // namespace bdpt
