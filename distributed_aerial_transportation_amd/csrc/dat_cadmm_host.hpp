// dat_cadmm_host.hpp -- the C-ADMM control step of one scenario on the host (control/rqp_cadmm.py:631-675): the
// lane functions of dat_cadmm_step.hpp in the drain's sequence (cadmm_drain<., false> then cadmm_drain<., true>,
// dat_cadmm_drain.hpp), a loop over the agents where the drain has lanes.  A plain host header, no HIP runtime: the
// CPU baseline (cpu_baseline/dat_cpu.hip) and the test-only host build (tests/hostsim, hs_cadmm_step) run it, and the
// GPU is checked against it (tests/test_gpu_parity.py, tests/test_gpu_c4_hard.py).
#pragma once

#include <climits>

#include "dat_cadmm_step.hpp"

namespace dat {

constexpr int CADMM_HOST_NMAX = 16;  // the largest team (NMAX, dat_kargs.hpp)

// What KArgs holds for the step, with the defaults dat_default_config and the handle give.  tail_prev / tail_pass:
// TAIL_PREV / TAIL_PASS with a forest, out of reach without one (cadmm_step_cfg).
struct CadmmStepCfg {
  double res_tol = 1e-2;
  int max_iter = 100;
  int use_total_res = 1;
  double rho0 = 1.0, tau = 1.0, rho_max = 2.0;
  double qp_tol = IPM_TOL;
  int tail_prev = INT_MAX, tail_pass = INT_MAX;
};
inline CadmmStepCfg cadmm_step_cfg(bool forest) {
  CadmmStepCfg c;
  if (forest) { c.tail_prev = TAIL_PREV; c.tail_pass = TAIL_PASS; }
  return c;
}

// One agent's env rows in slot form, as k_env_class leaves them for the drain.
struct CadmmEnvSlots {
  unsigned emask = 0;
  double lhs[DAT_NENV][3], rhs[DAT_NENV];
};
// The two front ends: from the scenario's forest (trees sorted by x, ntree x 3; none: no row) ...
inline void cadmm_env_of_trees(const double* prm, int n, const double* st, const double* trees, int ntree,
                               CadmmEnvSlots* env) {
  for (int i = 0; i < n; ++i) env_rows(prm, n, st, trees, ntree, i, prm[DAT_P_AENVD], &env[i].emask, env[i].lhs, env[i].rhs);
}
// ... and from the caller's compacted rows of one agent (nenv x 3, nenv <= DAT_NENV)
inline void cadmm_env_of_rows(const double* env_lhs, const double* env_rhs, int nenv, CadmmEnvSlots& env) {
  env.emask = env_slots_of_rows(env_lhs, env_rhs, nenv, env.lhs, env.rhs);
}

// The step's only hook: called once per agent-QP solve.  warm: the solve started from the agent's record.
struct CadmmNoObserver {
  void operator()(int /*pass*/, int /*agent*/, const QPLane<1>& /*lane*/, const IPMOut& /*o*/, bool /*warm*/) const {}
};

// One control step.  In: the parameter block, n, the state, acc_des (6), cfg, the agents' env rows (n).  In / out: the
// warm state cf (n x 3n), fbar (3n), lam (n x 3n) and *iters, the previous step's pass count in and this step's out.
// Out: f_des (3n), err_seq (max_iter + 1: the residuals of the passes that did not stop, KArgs::err's layout; may be
// null), qstatus (n: the agents' last QP status).  Every solve of a pass comes before the pass's consensus arithmetic
// (the drain's barrier).  The step keeps no global diagnostics: obs sees every solve.
template <class OBS = CadmmNoObserver>
inline void cadmm_host_step(const double* prm, int n, const double* st, const double* acc, const CadmmStepCfg& cfg,
                            const CadmmEnvSlots* env, double* cf, double* fbar, double* lam, int* iters, double* f_des,
                            double* err_seq, int* qstatus, OBS&& obs = OBS{}) {
  constexpr int RS = 7;  // the partials of one agent, as the drain's exchange slots (RDS, dat_cadmm_lds.hpp)
  const int N3 = 3 * n;
  const double* feq = prm + DAT_P_FEQ(n);
  QPShared S;
  build_shared(S, prm, n, st, acc, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, true);
  double Rt_all[CADMM_HOST_NMAX * 9], red[CADMM_HOST_NMAX * RS], wrec[CADMM_HOST_NMAX][WREC_SIZE];
  QPLane<1> P[CADMM_HOST_NMAX];
  EnvRows E[CADMM_HOST_NMAX];
  for (int i = 0; i < n; ++i) {
    make_Rt(prm + DAT_P_RCOM(n) + 3 * i, st + DAT_S_RL(n), Rt_all + 9 * i);
    lane_cadmm_static(P[i], prm, i);
    set_env_rows(P[i], E[i], S, env[i].emask, env[i].lhs, env[i].rhs);
    // rows certified infeasible are held (the tail certifies them once per scenario-step).  k_cadmm's passes run
    // uncertified: such a QP ends INACCURATE there and holds the previous solution too, but it is unclean, so the GPU
    // hands the scenario over in pass 0 and the tail owns every later pass, while `unclean` below stays false for it.
    // In that case the host keeps records later than the GPU; this difference from the drain remains.
    cadmm_certify_rows(P[i], PlainRef<QPShared>{&S}, EnvPlain{&E[i]});
    wrec[i][0] = 0.0;  // no recorded iterate yet
    qstatus[i] = ST_OPTIMAL;
  }
  const int prev_iter = *iters;
  double rho = cfg.rho0;
  int iter = 0;
  bool unclean = false;  // an earlier pass of the step had a redone solve
  for (;;) {
    const bool owns = tail_owns_pass(iter, prev_iter, cfg.tail_prev, cfg.tail_pass, unclean);
    const bool wson = tail_rule(iter, prev_iter, cfg.tail_prev, cfg.tail_pass);
    for (int i = 0; i < n; ++i) {
      lane_cadmm_dynamic(P[i], prm, n, i, Rt_all, lam + i * N3, fbar, rho);
      P[i].tuned = cadmm_tuned_start(iter, prev_iter);
      double y[1][3], w[6], best[best_size(1)];
      const bool warm = wson && wrec[i][0] == 1.0;
      const IPMOut o = ipm_solve_rows<MODE_CADMM, 1, IPM_FAST_REDO, true>(
          rows_needed(P[i].emask), PlainRef<QPShared>{&S}, EnvPlain{&E[i]}, RtPtr{Rt_all + 9 * i}, P[i], feq + 3 * i, y, w,
          best, IPM_MAX_ITER, cfg.qp_tol, wrec[i], wson);
      if (!tail_keeps_record(owns, o)) wrec[i][0] = 0.0;
      // IPMOut::stiff means "redone" only after a fast first attempt; a warm solve's first attempt is the robust one,
      // where it means stiff rows.  Harmless here: wson implies that the tail owns the pass already.
      unclean = unclean || o.stiff;  // (read by the passes after this one)
      qstatus[i] = o.status;
      obs(iter, i, P[i], o, warm);
      cadmm_take_solve(o, cf + i * N3, y[0], Rt_all, 9, lam + i * N3, fbar, rho, n, i, feq);
    }
    ++iter;
    rho = cadmm_next_rho(rho, cfg.tau, cfg.rho_max);
    for (int i = 0; i < n; ++i) cadmm_mean_block(cf, n, i, red + RS * i);
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < 3; ++c) fbar[3 * i + c] = red[RS * i + c];
    for (int i = 0; i < n; ++i) {
      if (cfg.use_total_res) red[RS * i + 6] = cadmm_total_res(cf + i * N3, fbar, n);
      else cadmm_aggregate_res(cf, cf + i * N3, Rt_all, 9, n, i, red + RS * i);
    }
    const double res = cadmm_pass_residual(red, RS, n, cfg.use_total_res);
    if (cadmm_stop(res, cfg.res_tol, iter, cfg.max_iter)) break;
    if (err_seq) err_seq[iter - 1] = res;
    for (int i = 0; i < n; ++i) cadmm_dual_update(lam + i * N3, cf + i * N3, fbar, rho, n);
  }
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) f_des[3 * i + c] = cf[i * N3 + 3 * i + c];  // f_app = diag copies (:669-671)
  *iters = iter;
}

}  // namespace dat
