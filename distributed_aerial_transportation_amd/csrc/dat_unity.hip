// dat_unity.hip -- the host units (dat.hip, dat_h_*.hip) and the kernel units beside them (dat_launch.hpp) as one
// translation unit, for the development builds whose device globals several kernel families write and dat.hip reads
// (-DDAT_PHASE_PROF, -DDAT_ITER_HIST, -DDAT_CAPTURE_LOOSE) and for A/B variants (tools/build_var.sh compiles this
// file).  Not part of the library's build (_lib.SRCS); its device code is that of the units, instruction for
// instruction (tools/same_kernels.py).
#define DAT_UNITY
#include "dat_k_cadmm.hip"
#include "dat_k_cadmm_adv.hip"
#include "dat_k_cadmm_tail.hip"
#include "dat_k_dd.hip"
#include "dat_k_step.hip"
#include "dat.hip"
#include "dat_h_ckpt.hip"
#include "dat_h_episode.hip"
#include "dat_h_log.hip"
