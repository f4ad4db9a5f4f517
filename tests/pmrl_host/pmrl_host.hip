// Host-side driver of the point-mass rigid-link step (TEST-ONLY): the serial forms pmrl_forward and pmrl_step of
// csrc/dat_pmrl_step.hpp, compiled with hipcc into tests/pmrl_host/libdat_pmrl_host.so and loaded only by tests/.
// They run the pieces a lane of k_pmrl_rollout / k_pmrl_forward runs, the links one after the other, so the reduced
// tension solve and the integration can be checked against the reference's fixture without a GPU.
#include "../../distributed_aerial_transportation_amd/csrc/dat_pmrl_step.hpp"

using namespace dat;

constexpr int PH_NMAX = 16;

extern "C" {

void ph_forward(const double* prm, int n, const double* st, const double* f, double* ddq, double* dvl, double* dwl,
                double* T) {
  pmrl_forward<PH_NMAX>(prm, n, st, f, ddq, dvl, dwl, T);
}

// `steps` steps of dt under the force f (3n, agent-major) held
void ph_steps(const double* prm, int n, double* st, int* counter, const double* f, double dt, int steps) {
  for (int s = 0; s < steps; ++s) pmrl_step<PH_NMAX>(prm, n, st, counter, f, dt);
}

// the reduced system of the state: S (packed upper, 21) and its right-hand side G y (6), for the conditioning figure
void ph_system(const double* prm, int n, const double* st, const double* f, double* S, double* Gy) {
  const double* Rl = st + DAT_S_RL(n);
  PmrlPayload p;
  pmrl_payload_terms(prm, Rl, st + DAT_S_WL(n), p);
  pmrl_system_clear(S, Gy);
  for (int i = 0; i < n; ++i) {
    PmrlLink lk;
    pmrl_link_terms(prm, n, i, p, Rl, st + DAT_S_Q(n) + 3 * i, st + DAT_S_DQ(n) + 3 * i, f + 3 * i, lk);
    pmrl_system_add(S, Gy, prm[DAT_P_PM_M(n) + i], lk.y, lk.g);
  }
}

}  // extern "C"
