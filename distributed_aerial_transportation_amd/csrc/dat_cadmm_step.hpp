// dat_cadmm_step.hpp -- the lane-level rules of the C-ADMM control step (control/rqp_cadmm.py:631-675), each
// stated once for every build that runs the step: the GPU drain (cadmm_drain, dat_cadmm_drain.hpp; k_agent_qp) and the
// host step (cadmm_host_step, dat_cadmm_host.hpp: the CPU baseline cpu_baseline/dat_cpu.hip and the test-only host
// build tests/hostsim run it).  A GPU lane calls them for its agent i between the drain's barriers; the host step
// calls them in a loop over i < n.  Every floating-point
// expression stands whole inside one function: with -ffp-contract=on (multiply-adds fused within an expression
// only) an inlined copy computes the same bits at every call site.
#pragma once

#include "dat_qp.hpp"

namespace dat {

// ------------------------------------------------------------------ the tail rule
// (TAIL_PREV, TAIL_PASS and what the rule is for: dat_qp.hpp)
// tail_prev / tail_pass: TAIL_PREV / TAIL_PASS with a forest, out of reach (INT_MAX) without one.
// Wedged before the step: the whole step is the tail's (k_env_class routes it there, or k_cadmm hands it over
// before its first pass).
DAT_HD bool tail_wedged(int prev_iter, int tail_prev) { return prev_iter > tail_prev; }
// The rule names pass p: warm start and stall exit in that pass; k_cadmm hands the scenario over before it.
DAT_HD bool tail_rule(int pass, int prev_iter, int tail_prev, int tail_pass) {
  return pass >= 1 && (tail_wedged(prev_iter, tail_prev) || pass >= tail_pass);
}
// Which agent QPs leave a warm-start record, as k_cadmm and k_cadmm_tail between them apply it: the tail records
// every solve it runs, k_cadmm none.  The tail owns pass p -- it runs all of the pass's solves -- when the step was
// wedged from its start, when p >= tail_pass, or when an earlier pass of the step was unclean (k_cadmm handed the
// scenario over there).
DAT_HD bool tail_owns_pass(int pass, int prev_iter, int tail_prev, int tail_pass, bool unclean_before) {
  return tail_wedged(prev_iter, tail_prev) || pass >= tail_pass || unclean_before;
}
// Agent i's record of pass p is kept when the tail owns p, or when i's own solve in p was redone (IPMOut::stiff of
// IPM_FAST_REDO: its fast attempt was unclean, so k_cadmm hands that solve over and the tail runs it again with the
// record).  The host step (dat_cadmm_host.hpp) solves with a record buffer in every pass and drops the records this
// rule does not keep; a record is read only under tail_rule, in a pass the tail owns.
DAT_HD bool tail_keeps_record(bool owns_pass, const IPMOut& o) { return owns_pass || o.stiff != 0; }
// The IPM's tuned start (ipm_solve): the step's first pass, or the warm closed-loop regime.
DAT_HD bool cadmm_tuned_start(int pass, int prev_iter) { return pass == 0 || prev_iter <= 3; }

// ------------------------------------------------------------------ the copy of a solve
// Agent i's copy f (3n, agent-major) of an OPTIMAL solve: its own block y, the others' free blocks from the
// solve's u-space gradient pi.  Rt_all: n matrices rt_stride doubles apart (RT_STRIDE in LDS, 9 on the host);
// lam, fbar: the agent's multipliers and the mean (3n).
DAT_HD void cadmm_copy_of_solve(double* f, const double* y, const double* pi, const double* Rt_all, int rt_stride,
                                const double* lam, const double* fbar, double rho, int n, int i) {
  for (int j = 0; j < n; ++j) {
    if (j == i) {
      f[3 * j] = y[0]; f[3 * j + 1] = y[1]; f[3 * j + 2] = y[2];
    } else {
      cadmm_free_block(Rt_all + rt_stride * j, lam + 3 * j, fbar + 3 * j, pi, rho, f + 3 * j);
    }
  }
}
// What a solve's status does to the agent's copy (RQPPrimalSolver.solve): OPTIMAL takes the solution, a solver
// exception f_eq (control/rqp_cadmm.py:491-494), anything else holds the previous copy (:496-499).
DAT_HD void cadmm_take_solve(const IPMOut& o, double* f, const double* y, const double* Rt_all, int rt_stride,
                             const double* lam, const double* fbar, double rho, int n, int i, const double* feq) {
  if (o.status == ST_OPTIMAL) {
    cadmm_copy_of_solve(f, y, o.pi, Rt_all, rt_stride, lam, fbar, rho, n, i);
  } else if (o.status == ST_FAILED) {
    for (int c = 0; c < 3 * n; ++c) f[c] = feq[c];
  }
}

// ------------------------------------------------------------------ the pass's consensus arithmetic
// cfs: the scenario's n copies (n x 3n); f: agent i's own copy; fbar: the mean (3n).
// Block i of the consensus mean, summed in agent order like the reference (control/rqp_cadmm.py:591-600);
// agent-major: the three components of copy k read together (same per-component order).
DAT_HD void cadmm_mean_block(const double* cfs, int n, int i, double* out) {
  const int N3 = 3 * n;
  double s3[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < n; ++k) {
    const double* ck = cfs + k * N3 + 3 * i;
    const double c0 = ck[0], c1 = ck[1], c2 = ck[2];
    s3[0] += c0; s3[1] += c1; s3[2] += c2;
  }
  for (int c = 0; c < 3; ++c) out[c] = s3[c] / n;
}
// Total residual: the largest of the three row sums of |f - fbar| of one copy (the matrix inf-norm of the copy's
// rows, control/rqp_cadmm.py:582-600); the pass's residual is the largest over the copies.
DAT_HD double cadmm_total_res(const double* f, const double* fbar, int n) {
  double rmax = 0.0;
  double s3[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < n; ++j) {
    const double m0 = f[3 * j], m1 = f[3 * j + 1], m2 = f[3 * j + 2];
    s3[0] += fabs(m0 - fbar[3 * j]);
    s3[1] += fabs(m1 - fbar[3 * j + 1]);
    s3[2] += fabs(m2 - fbar[3 * j + 2]);
  }
  for (int r = 0; r < 3; ++r) rmax = fmax(rmax, s3[r]);
  return rmax;
}
// Aggregate residual (control/rqp_cadmm.py:602-621): the own copy's force / moment totals of the others,
// E_F,i = F_i - (sum_k f_app_k - f_app_i), E_M,i likewise with moments of f_app (FM: F (3), then M (3)).
DAT_HD void cadmm_aggregate_res(const double* cfs, const double* f, const double* Rt_all, int rt_stride, int n, int i,
                                double* FM) {
  const int N3 = 3 * n;
  double F[3] = {0, 0, 0}, M[3] = {0, 0, 0};
  for (int j = 0; j < n; ++j) {
    if (j == i) continue;
    double m3[3];
    mv3(Rt_all + rt_stride * j, f + 3 * j, m3);
    for (int c = 0; c < 3; ++c) { F[c] += f[3 * j + c]; M[c] += m3[c]; }
  }
  for (int k = 0; k < n; ++k) {
    if (k == i) continue;
    const double* fk = cfs + k * N3 + 3 * k;  // f_app_k = agent k's own block
    double m3[3];
    mv3(Rt_all + rt_stride * k, fk, m3);
    for (int c = 0; c < 3; ++c) { F[c] -= fk[c]; M[c] -= m3[c]; }
  }
  for (int c = 0; c < 3; ++c) { FM[c] = F[c]; FM[3 + c] = M[c]; }
}
// Dual update of one agent's multipliers (control/rqp_cadmm.py:627-629).
DAT_HD void cadmm_dual_update(double* lam, const double* f, const double* fbar, double rho, int n) {
  for (int c = 0; c < 3 * n; ++c) lam[c] += rho * (f[c] - fbar[c]);
}
// The pass's residual from the agents' partials (red: n records `stride` doubles apart -- the aggregate's F / M
// totals at [0, 6), the total residual at [6]; one lane of the slot reduces them): the largest total residual, or
// for the aggregate the largest row sum of |E_F| and of |E_M| (control/rqp_cadmm.py:582-621).
DAT_HD double cadmm_pass_residual(const double* red, int stride, int n, bool use_total_res) {
  double res = 0.0;
  if (use_total_res) {
    for (int k = 0; k < n; ++k) res = fmax(res, red[stride * k + 6]);
  } else {
    for (int r = 0; r < 3; ++r) {
      double sF = 0.0, sM = 0.0;
      for (int k = 0; k < n; ++k) {
        sF += fabs(red[stride * k + r]);
        sM += fabs(red[stride * k + 3 + r]);
      }
      res = fmax(res, fmax(sF, sM));
    }
  }
  return res;
}
// The stop test after `iter` passes (control/rqp_cadmm.py:661) and the next pass's rho (:657-658).  (res_tol and
// max_iter by reference: the drain reads KArgs::max_iter only where the first test fails, as its inline text did;
// by value the kernels' code changes.)
DAT_HD bool cadmm_stop(double res, const double& res_tol, int iter, const int& max_iter) {
  return (res < res_tol) || (iter > max_iter);
}
DAT_HD double cadmm_next_rho(double rho, double tau, double rho_max) { return fmin(rho * tau, rho_max); }

// ------------------------------------------------------------------ the agent QP from caller-supplied rows
// compacted rows (nenv x 3, nenv: slots 0 .. nenv - 1) -> slot arrays; returns the slot mask
DAT_HD unsigned env_slots_of_rows(const double* env_lhs, const double* env_rhs, int nenv, double lhs[DAT_NENV][3],
                                  double rhs[DAT_NENV]) {
  for (int r = 0; r < DAT_NENV; ++r) {
    for (int c = 0; c < 3; ++c) lhs[r][c] = r < nenv ? env_lhs[3 * r + c] : 0.0;
    rhs[r] = r < nenv ? env_rhs[r] : 0.0;
  }
  return (1u << nenv) - 1u;
}
// The certificate of infeasible rows as the closed loop applies it (k_cadmm_tail, once per scenario-step): rows
// certified infeasible are held.  True when this call certified them.
template <class SH, class ER>
DAT_HD bool cadmm_certify_rows(QPLane<1>& P, const SH& sh, const ER& er) {
  const bool cert = !P.infeasible && dvl_rows_infeasible(sh, er, P.emask);
  if (cert) P.infeasible = 1;
  return cert;
}
// Agent i's lane (after lane_cadmm_static) and env rows from the caller's compacted rows and the pass's
// multipliers, mean and rho; the certificate is the caller's (one ipm_attempt is probed without it).
DAT_HD void cadmm_lane_of_rows(QPLane<1>& P, EnvRows& E, const QPShared& S, const double* prm, int n, int i,
                               const double* Rt_all, const double* env_lhs, const double* env_rhs, int nenv,
                               const double* lam, const double* fbar, double rho) {
  double lhs[DAT_NENV][3], rhs[DAT_NENV];
  const unsigned mask = env_slots_of_rows(env_lhs, env_rhs, nenv, lhs, rhs);
  set_env_rows(P, E, S, mask, lhs, rhs);
  lane_cadmm_dynamic(P, prm, n, i, Rt_all, lam, fbar, rho);
}

}  // namespace dat
