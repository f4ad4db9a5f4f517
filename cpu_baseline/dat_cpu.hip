// dat_cpu.hip -- the CPU baseline of bench.py: the C4 closed loop on the host's cores.
//
// SURVEY.md 8(d) "CPU baseline plan": the reference's cvxpy + Clarabel path cannot run here or on
// the GPU box, so the reported CPU baseline is a C++ fp64 restatement of the same controller loop,
// one scenario per OpenMP thread, compiled -O3 for x86-64-v3 (AVX2 / FMA; built in the dev
// container, run on the GPU box's host).  Per scenario and high-level step it runs what the GPU
// runs:
//   desired acceleration (example/rqp_example.py:33-59)                       desired_accel_forest
//   RQPCADMMController.control (control/rqp_cadmm.py:631-675): per agent the env CBF rows
//     (:307-373, env_rows), RQPPrimalSolver.solve (:482-501, ipm_solve), consensus mean and the
//     matrix inf-norm residual (:582-600), dual update (:627-629); warm f, f_mean, lambda persist
//   hl_every simulation steps: LL SO(3) PD + dynamics + integration (sim_step)
// using the same per-lane __host__ __device__ functions as the kernels (dat_core.hpp / dat_qp.hpp),
// so the CPU and GPU do identical arithmetic per scenario.  This is a measured baseline, not the
// product: the package never loads it.
#include <omp.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../distributed_aerial_transportation_amd/csrc/dat_cadmm_host.hpp"

using namespace dat;

#if defined(DAT_IPM_STATS)
long long g_ith[2][8][32];  // tools/ipm_stats.py: IPM iterations by start and active env rows
#endif

namespace {
constexpr int NMAXC = CADMM_HOST_NMAX;

struct Ctx {
  int n, B, P, S;
  std::vector<double> params, state, cf, cfbar, clam, fdes, trees, mountain;
  std::vector<int> counter, tree_off, scen_forest, iters;
  int nforest = 0;
  long long qp = 0, ipm = 0;
};

// One C-ADMM control step of scenario sc: the desired acceleration, then the host step (dat_cadmm_host.hpp) on the
// scenario's forest, with the defaults of dat_default_config and the GPU's tail rule.
void cadmm_step(Ctx& c, int sc, long long* qp, long long* ipm) {
  const int n = c.n, N3 = 3 * n;
  const double* prm = c.params.data();
  const double* st = c.state.data() + (size_t)sc * c.S;
  const double* trees = nullptr;
  int nt = 0;
  const double* mnt = nullptr;
  const double m0[DAT_MOUNTAIN_SIZE] = {30.0, 0.0, 25.0, 1e300, 0.0};
  if (c.nforest > 0) {
    const int f = c.scen_forest.empty() ? 0 : c.scen_forest[sc];
    trees = c.trees.data() + 3 * (size_t)c.tree_off[f];
    nt = c.tree_off[f + 1] - c.tree_off[f];
    mnt = c.mountain.data() + (size_t)f * DAT_MOUNTAIN_SIZE;
  }
  double acc[6];
  desired_accel_forest(st, n, mnt ? mnt : m0, 1.5, acc);
  CadmmEnvSlots env[NMAXC];
  cadmm_env_of_trees(prm, n, st, trees, nt, env);
  int qstatus[NMAXC];
  cadmm_host_step(prm, n, st, acc, cadmm_step_cfg(c.nforest > 0), env, c.cf.data() + (size_t)sc * n * N3,
                  c.cfbar.data() + (size_t)sc * N3, c.clam.data() + (size_t)sc * n * N3, &c.iters[sc],
                  c.fdes.data() + (size_t)sc * N3, nullptr, qstatus,
                  [&](int, int, const QPLane<1>& P, const IPMOut& o, bool) {
                    ++*qp;
                    *ipm += o.iters;
#if defined(DAT_IPM_STATS)
                    ++g_ith[P.tuned ? 1 : 0][__builtin_popcount(P.emask) & 7][o.iters < 31 ? o.iters : 31];
#else
                    (void)P;
#endif
                  });
}
}  // namespace

extern "C" {

#if defined(DAT_IPM_STATS) && !defined(__HIP_DEVICE_COMPILE__)
void datcpu_ipm_ith(long long* out) {  // [tuned start][active env rows][IPM iterations] solves
  long long* g = &g_ith[0][0][0];
  for (int k = 0; k < 512; ++k) { out[k] = g[k]; g[k] = 0; }
}
void datcpu_ipm_stats(long long* out) {
  for (int k = 0; k < 16; ++k) { out[k] = dat::g_ipm_stats[k]; dat::g_ipm_stats[k] = 0; }
  for (int k = 0; k < 72; ++k) { out[16 + k] = dat::g_ipm_hist[k / 24][k % 24]; dat::g_ipm_hist[k / 24][k % 24] = 0; }
}
#endif

void* datcpu_create(int n, int B, const double* params) {
  if (n < 3 || n > NMAXC || B < 1 || !params) return nullptr;
  Ctx* c = new Ctx();
  c->n = n;
  c->B = B;
  c->P = DAT_PARAM_SIZE(n);
  c->S = DAT_STATE_SIZE(n);
  c->params.assign(params, params + c->P);
  const size_t N3 = 3 * (size_t)n;
  c->state.assign((size_t)B * c->S, 0.0);
  c->counter.assign(B, 0);
  c->iters.assign(B, 0);
  c->fdes.assign((size_t)B * N3, 0.0);
  c->cf.assign((size_t)B * n * N3, 0.0);
  c->cfbar.assign((size_t)B * N3, 0.0);
  c->clam.assign((size_t)B * n * N3, 0.0);
  const double* feq = params + DAT_P_FEQ(n);
  for (int b = 0; b < B; ++b) {  // warm start f = f_mean = f_eq, lambda = 0 (control/rqp_cadmm.py:577-580)
    for (int i = 0; i < n; ++i) std::memcpy(&c->cf[((size_t)b * n + i) * N3], feq, sizeof(double) * N3);
    std::memcpy(&c->cfbar[(size_t)b * N3], feq, sizeof(double) * N3);
    std::memcpy(&c->fdes[(size_t)b * N3], feq, sizeof(double) * N3);
  }
  return c;
}

void datcpu_destroy(void* h) { delete (Ctx*)h; }

// trees of each forest must be sorted by x (as dat_set_forests stores them for the GPU)
int datcpu_set_forests(void* h, int num_forests, const int* tree_offsets, const double* tree_pos,
                       const int* scenario_forest, const double* mountain) {
  Ctx* c = (Ctx*)h;
  if (!c || num_forests < 0) return -1;
  c->nforest = num_forests;
  if (num_forests == 0) return 0;
  const int T = tree_offsets[num_forests];
  c->tree_off.assign(tree_offsets, tree_offsets + num_forests + 1);
  c->trees.assign(tree_pos, tree_pos + 3 * (size_t)T);
  c->mountain.assign(mountain, mountain + (size_t)num_forests * DAT_MOUNTAIN_SIZE);
  if (scenario_forest) c->scen_forest.assign(scenario_forest, scenario_forest + c->B);
  return 0;
}

int datcpu_set_state(void* h, const double* state) {
  Ctx* c = (Ctx*)h;
  if (!c || !state) return -1;
  c->state.assign(state, state + (size_t)c->B * c->S);
  std::fill(c->counter.begin(), c->counter.end(), 0);
  return 0;
}

// the constructor's warm state (f = f_mean = f_eq, lambda = 0, control/rqp_cadmm.py:577-580) and no
// step history (the previous step's ADMM iteration count selects the IPM start, as on the GPU: k_warm)
int datcpu_reset_warm(void* h) {
  Ctx* c = (Ctx*)h;
  if (!c) return -1;
  const size_t N3 = 3 * (size_t)c->n;
  const double* feq = c->params.data() + DAT_P_FEQ(c->n);
  std::fill(c->clam.begin(), c->clam.end(), 0.0);
  std::fill(c->iters.begin(), c->iters.end(), 0);
  for (int b = 0; b < c->B; ++b) {
    for (int i = 0; i < c->n; ++i) std::memcpy(&c->cf[((size_t)b * c->n + i) * N3], feq, sizeof(double) * N3);
    std::memcpy(&c->cfbar[(size_t)b * N3], feq, sizeof(double) * N3);
    std::memcpy(&c->fdes[(size_t)b * N3], feq, sizeof(double) * N3);
  }
  return 0;
}

// hl_steps closed-loop periods of scenarios [first, first + count) on `threads` OpenMP threads (0:
// default); returns the agent-QP solves and IPM iterations of the call.
int datcpu_closed_loop(void* h, int hl_steps, int first, int count, int threads, int hl_every, double dt,
                       long long* qp_solves, long long* ipm_iters) {
  Ctx* c = (Ctx*)h;
  if (!c || first < 0 || count < 0 || first + count > c->B) return -1;
  long long qp = 0, ipm = 0;
  if (threads <= 0) threads = omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) reduction(+ : qp, ipm)
  for (int sc = first; sc < first + count; ++sc) {
    for (int k = 0; k < hl_steps; ++k) {
      cadmm_step(*c, sc, &qp, &ipm);
      double* st = c->state.data() + (size_t)sc * c->S;
      const double* fd = c->fdes.data() + (size_t)sc * 3 * c->n;
      for (int s = 0; s < hl_every; ++s) sim_step<NMAXC>(c->params.data(), c->n, st, &c->counter[sc], fd, dt);
    }
  }
  if (qp_solves) *qp_solves = qp;
  if (ipm_iters) *ipm_iters = ipm;
  return 0;
}

int datcpu_get(void* h, double* state, double* f_des, int* iters) {
  Ctx* c = (Ctx*)h;
  if (!c) return -1;
  if (state) std::memcpy(state, c->state.data(), sizeof(double) * c->state.size());
  if (f_des) std::memcpy(f_des, c->fdes.data(), sizeof(double) * c->fdes.size());
  if (iters) std::memcpy(iters, c->iters.data(), sizeof(int) * c->iters.size());
  return 0;
}

int datcpu_max_threads(void) { return omp_get_max_threads(); }

}  // extern "C"
