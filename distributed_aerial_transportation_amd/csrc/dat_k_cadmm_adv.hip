// dat_k_cadmm_adv.hip -- the C-ADMM drain kernels of the closed loop's advance overlap, k_cadmm<true, .> and
// k_cadmm0<true, .> (write-through outputs, done stamps, the queue-empty word), one per row-mode word:
// dat_cadmm_drain.hpp, instantiated here,
// and with them the DD drain with a forest, k_dd<true> (dat_dd_drain.hpp).  A quarter of the library's device code,
// in a unit of its own (dat_launch.hpp: the units, and why k_dd is here).
#include <hip/hip_runtime.h>

#include "dat_cadmm_drain.hpp"
#include "dat_dd_drain.hpp"
#include "dat_launch.hpp"

namespace dat {

hipError_t launch_k_cadmm_adv(bool forest, int rms, int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  return launch_k_cadmm_of<true>(forest, rms, blocks, lds, st, a);
}
// the DD drain with a forest (this unit's caller of build_shared: dat_launch.hpp)
hipError_t launch_k_dd_env(int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  hipLaunchKernelGGL(k_dd<true>, dim3(blocks), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace dat
