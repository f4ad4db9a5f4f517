// dat_k_cadmm.hip -- the C-ADMM drain kernels of a plain control step, k_cadmm<false> (with a forest: env classes 3,
// 2, 1, 0) and k_cadmm0<false> (without one): dat_cadmm_drain.hpp, instantiated here, and with them the DD drain
// without a forest, k_dd<false> (dat_dd_drain.hpp).  A quarter of the library's device code, in a unit of its own
// (dat_launch.hpp: the units, and why k_dd is here).
#include <hip/hip_runtime.h>

#include "dat_cadmm_drain.hpp"
#include "dat_dd_drain.hpp"
#include "dat_launch.hpp"

namespace dat {

hipError_t launch_k_cadmm(bool forest, int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  hipLaunchKernelGGL(forest ? k_cadmm<false> : k_cadmm0<false>, dim3(blocks), dim3(64), lds, st, a);
  return hipGetLastError();
}
// the DD drain without a forest (this unit's caller of build_shared with cadmm = false: dat_launch.hpp)
hipError_t launch_k_dd(int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  hipLaunchKernelGGL(k_dd<false>, dim3(blocks), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace dat
