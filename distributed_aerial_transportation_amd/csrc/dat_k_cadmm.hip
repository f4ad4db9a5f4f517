// dat_k_cadmm.hip -- the C-ADMM drain kernels of a plain control step, k_cadmm<false, .> (with a forest: env classes 3,
// 2, 1, 0) and k_cadmm0<false, .> (without one), one per row-mode word: dat_cadmm_drain.hpp, instantiated here, and with them the DD drain
// without a forest, k_dd<false> (dat_dd_drain.hpp).  A quarter of the library's device code, in a unit of its own
// (dat_launch.hpp: the units, and why k_dd is here).
#include <hip/hip_runtime.h>

#include "dat_cadmm_drain.hpp"
#include "dat_dd_drain.hpp"
#include "dat_launch.hpp"

namespace dat {

hipError_t launch_k_cadmm(bool forest, int rms, int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  return launch_k_cadmm_of<false>(forest, rms, blocks, lds, st, a);
}
// the DD drain without a forest (this unit's caller of build_shared: dat_launch.hpp)
hipError_t launch_k_dd(int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  hipLaunchKernelGGL(k_dd<false>, dim3(blocks), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace dat
