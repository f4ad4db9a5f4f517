// Host-side driver of the per-lane device functions in dat_core.hpp (TEST-ONLY).
//
// Compiled with hipcc into tests/hostsim/libdat_hostsim.so and loaded only by tests/ (never by
// the product package): it runs the exact __host__ __device__ code of one GPU lane on the CPU so
// the reduced-QP algebra, the env rows and the rollout can be checked against the oracle in the
// dev container, which has no GPU.  The product path has no CPU fallback.
#include <vector>

#include "../../distributed_aerial_transportation_amd/csrc/dat_cadmm_host.hpp"
#include "../../distributed_aerial_transportation_amd/csrc/dat_dd_step.hpp"

using namespace dat;

#ifndef HS_TOL
#define HS_TOL 1e-10
#endif

namespace {
// diagnostics of the last solve (hs_last_diag)
double g_merit = 0.0;
int g_inband = 0, g_why = 0;
int g_refs = 0, g_corrs = 0;
void diag(const IPMOut& o) {
  g_merit = o.merit;
  g_inband = o.inband;
  g_why = o.why;
  g_refs = o.refs;
  g_corrs = o.corrs;
}

// stiff exits of the fast solver since the last call (the redo count of IPM_FAST_REDO), and whether the last
// solve was redone robustly (its fast attempt was not clean)
long long g_stiff_redo = 0;
int g_last_stiff = 0;

// The C-ADMM agent QP of agent i from the caller's compacted rows, as one GPU lane sets it up and copies it out
// (dat_cadmm_step.hpp).  HS_SOLVE: the GPU's definition (k_cadmm / k_cadmm_tail: rows certified infeasible are
// held; the fast solver, redone robustly when not clean); HS_WARM: the same with the tail kernel's warm-start
// record wrec (in / out) and, wson, the warm first attempt and the stall exit; HS_ATTEMPT: one ipm_attempt, no
// certificate (arg0: the robust instantiation, arg1: the start)
enum HsSolve { HS_SOLVE, HS_WARM, HS_ATTEMPT };
int cadmm_qp(HsSolve how, const double* prm, int n, const double* st, const double* acc, const double* env_lhs,
             const double* env_rhs, int nenv, int i, const double* lam, const double* fbar, double rho, int arg0,
             int arg1, double* wrec, double* f_out, int* iters, int* inband) {
  if (nenv > DAT_NENV) return -1;
  double Rt_all[16 * 9];
  for (int j = 0; j < n; ++j) make_Rt(prm + DAT_P_RCOM(n) + 3 * j, st + DAT_S_RL(n), Rt_all + 9 * j);
  QPShared S;
  build_shared(S, prm, n, st, acc, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, true);
  QPLane<1> P;
  lane_cadmm_static(P, prm, i);
  EnvRows E;
  cadmm_lane_of_rows(P, E, S, prm, n, i, Rt_all, env_lhs, env_rhs, nenv, lam, fbar, rho);
  const PlainRef<QPShared> sh{&S};
  const EnvPlain er{&E};
  const RtPtr rt{Rt_all + 9 * i};
  const double* y0 = prm + DAT_P_FEQ(n) + 3 * i;
  double y[1][3], w[6], best[best_size(1)];
  IPMOut o;
  if (how == HS_ATTEMPT) {
    o = arg0 ? ipm_attempt<MODE_CADMM, 1, DAT_MAXROW, PlainRef<QPShared>, EnvPlain, RtPtr, RowRegs, 0, NoGrp, true>(
                   sh, er, rt, P, y0, y, w, best, 50, HS_TOL, RowRegs{}, NoGrp{}, arg1)
             : ipm_attempt<MODE_CADMM, 1, DAT_MAXROW, PlainRef<QPShared>, EnvPlain, RtPtr, RowRegs, 0, NoGrp, false>(
                   sh, er, rt, P, y0, y, w, best, 50, HS_TOL, RowRegs{}, NoGrp{}, arg1);
  } else {
    P.tuned = arg0;
    cadmm_certify_rows(P, sh, er);
    const int nr = rows_needed(P.emask);
    o = how == HS_WARM
            ? ipm_solve_rows<MODE_CADMM, 1, IPM_FAST_REDO, true>(nr, sh, er, rt, P, y0, y, w, best, 50, HS_TOL, wrec,
                                                                 arg1 != 0)
            : ipm_solve_rows<MODE_CADMM, 1, IPM_FAST_REDO>(nr, sh, er, rt, P, y0, y, w, best, 50, HS_TOL);
    if (o.stiff) ++g_stiff_redo;
    g_last_stiff = o.stiff;
    *inband = o.inband ? 10 * o.why + 1 : 0;
  }
  diag(o);
  cadmm_copy_of_solve(f_out, y[0], o.pi, Rt_all, 9, lam, fbar, rho, n, i);
  *iters = o.iters;
  return o.status;
}

template <int NB>
int cent_nb_(const double* prm, const double* st, const double* acc, const double* env_lhs, const double* env_rhs,
            int nenv, double* f_out, int* iters) {
  QPShared S;
  build_shared(S, prm, NB, st, acc, prm[DAT_P_KFC], prm[DAT_P_KMC], 2, false);
  QPLane<NB> P;
  double Rt[NB][9];
  lane_cent(P, prm, NB, st, Rt);
  double lhs[DAT_NENV][3], rhs[DAT_NENV];
  const unsigned mask = env_slots_of_rows(env_lhs, env_rhs, nenv, lhs, rhs);
  EnvRows E;
  set_env_rows(P, E, S, mask, lhs, rhs);
  double y[NB][3], w[6], best[best_size(NB)];
  IPMOut o = ipm_solve_rows<MODE_CENT, NB>(rows_needed(P.emask), PlainRef<QPShared>{&S}, EnvPlain{&E},
                                           RtPtr{&Rt[0][0]}, P, prm + DAT_P_FEQ(NB), y, w, best, 50, HS_TOL);
  diag(o);
  for (int k = 0; k < NB; ++k)
    for (int c = 0; c < 3; ++c) f_out[3 * k + c] = y[k][c];
  *iters = o.iters;
  return o.status;
}

}  // namespace

extern "C" {

// refinement passes run and corrections applied by the last solve
void hs_last_work(int* refs, int* corrs) {
  *refs = g_refs;
  *corrs = g_corrs;
}
void hs_last_diag(double* merit, int* inband, int* why) {
  *merit = g_merit;
  *inband = g_inband;
  *why = g_why;
}

long long hs_stiff_redos() { return g_stiff_redo; }
int hs_last_stiff() { return g_last_stiff; }

// as hs_qp_cadmm with k_cadmm's IPM start policy flag (P.tuned) and the in-band exit flag out
int hs_qp_cadmm_ex(const double* prm, int n, const double* st, const double* acc, const double* env_lhs,
                   const double* env_rhs, int nenv, int i, const double* lam, const double* fbar, double rho,
                   int tuned, double* f_out, int* iters, int* inband) {
  return cadmm_qp(HS_SOLVE, prm, n, st, acc, env_lhs, env_rhs, nenv, i, lam, fbar, rho, tuned, 0, nullptr, f_out, iters,
                  inband);
}
int hs_qp_cadmm(const double* prm, int n, const double* st, const double* acc, const double* env_lhs,
                const double* env_rhs, int nenv, int i, const double* lam, const double* fbar, double rho,
                double* f_out, int* iters) {
  int ib = 0;
  return hs_qp_cadmm_ex(prm, n, st, acc, env_lhs, env_rhs, nenv, i, lam, fbar, rho, 0, f_out, iters, &ib);
}
// as hs_qp_cadmm_ex with the tail kernel's agent QP: the warm-start record (wrec: WREC_SIZE doubles, in / out: the
// converged iterate is recorded) and, wson != 0, the warm first attempt (when wrec[0] = 1) and the stall exit
int hs_qp_cadmm_warm(const double* prm, int n, const double* st, const double* acc, const double* env_lhs,
                     const double* env_rhs, int nenv, int i, const double* lam, const double* fbar, double rho,
                     int tuned, double* wrec, int wson, double* f_out, int* iters, int* inband) {
  return cadmm_qp(HS_WARM, prm, n, st, acc, env_lhs, env_rhs, nenv, i, lam, fbar, rho, tuned, wson, wrec, f_out, iters,
                  inband);
}
// one ipm_attempt of the C-ADMM agent QP (development: tools/loose_probe.py): rob selects the robust
// instantiation, start the initial point (0 conservative, 1 tuned, 2 conservative x 10)
int hs_qp_cadmm_attempt(const double* prm, int n, const double* st, const double* acc, const double* env_lhs,
                        const double* env_rhs, int nenv, int i, const double* lam, const double* fbar, double rho,
                        int rob, int start, double* f_out, int* iters) {
  int ib = 0;
  return cadmm_qp(HS_ATTEMPT, prm, n, st, acc, env_lhs, env_rhs, nenv, i, lam, fbar, rho, rob, start, nullptr, f_out,
                  iters, &ib);
}

int hs_qp_dd(const double* prm, int n, const double* st, const double* acc, const double* env_lhs,
             const double* env_rhs, int nenv, int i, const double* c9, double* x_out, int* iters) {
  if (nenv > DAT_NENV) return -1;
  double Rt[9];
  make_Rt(prm + DAT_P_RCOM(n) + 3 * i, st + DAT_S_RL(n), Rt);
  QPShared S;
  build_shared(S, prm, n, st, acc, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, false);
  QPLane<1> P;
  lane_dd_static(P, prm, i);
  set_dd_price(P, prm, n, i, c9);
  double lhs[DAT_NENV][3], rhs[DAT_NENV];
  const unsigned mask = env_slots_of_rows(env_lhs, env_rhs, nenv, lhs, rhs);
  EnvRows E;
  set_env_rows(P, E, S, mask, lhs, rhs);
  double y[1][3], w[6], best[best_size(1)];
  IPMOut o = ipm_solve_rows<MODE_DD, 1>(rows_needed(P.emask), PlainRef<QPShared>{&S}, EnvPlain{&E},
                                        RtPtr{Rt}, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, best, 50, HS_TOL);
  diag(o);
  for (int c = 0; c < 3; ++c) x_out[c] = y[0][c];
  for (int c = 0; c < 6; ++c) x_out[3 + c] = w[c];
  *iters = o.iters;
  return o.status;
}

// H^-1 of one scenario's DD quasi-Newton matrix (N x N row-major, N = 6n), as k_dd_setup computes it: the
// header's element steps (dat_dd_step.hpp) in the serial order the kernel's lanes reproduce
void hs_dd_setup(const double* prm, int n, const double* st, double* Hinv) {
  const int N = 6 * n;
  std::vector<double> Qi(81 * n), Rts(9 * n), H(2 * N * N), fac(N);
  for (int j = 0; j < n; ++j) {
    double Q[81], A[162], colk[9];
    dd_strong_convexity(prm, n, st, j, Q);
    dd_qinv_augment(Q, A);
    make_Rt(prm + DAT_P_RCOM(n) + 3 * j, st + DAT_S_RL(n), Rts.data() + 9 * j);
    for (int k = 0; k < 9; ++k) {
      const int p = dd_qinv_pivot_row(A, k);
      for (int c = 0; c < 18; ++c) dd_qinv_exchange(A, k, p, c);
      for (int r = 0; r < 9; ++r) colk[r] = A[18 * r + k];
      for (int c = 0; c < 18; ++c) dd_qinv_update_col(A, colk, k, c);
    }
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) Qi[81 * j + 9 * r + c] = dd_qinv_sym(A, r, c);
  }
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) {
      H[2 * N * r + c] = dd_h_element(Qi.data(), Rts.data(), n, r, c);
      H[2 * N * r + N + c] = (r == c) ? 1.0 : 0.0;
    }
  for (int k = 0; k < N; ++k) {
    const double piv = H[2 * N * k + k];
    for (int r = 0; r < N; ++r) fac[r] = H[2 * N * r + k];
    for (int c = 0; c < 2 * N; ++c) dd_hinv_update_col(H.data(), 2 * N, N, fac.data(), piv, k, c);
  }
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) Hinv[N * r + c] = H[2 * N * r + N + c];
}

// a DD controller's warm state before its first step, as k_warm sets it (that kernel is not the DD step's and keeps
// its own lines): zero multipliers, every agent holding dd_fallback over the sum of f_eq
void hs_dd_warm_reset(const double* prm, int n, double* lamF, double* lamM, double* prev) {
  const double* feq = prm + DAT_P_FEQ(n);
  double s3[3] = {0, 0, 0};
  for (int k = 0; k < n; ++k)
    for (int c = 0; c < 3; ++c) s3[c] += feq[3 * k + c];
  for (int c = 0; c < 3 * n; ++c) { lamF[c] = 0.0; lamM[c] = 0.0; }
  for (int i = 0; i < n; ++i) dd_fallback(prm, n, i, s3, prev + 9 * i);
}

// One DD control step of one scenario in k_dd's sequence, a loop over the agents where the kernel has lanes: every
// agent's solve of a pass comes before any write of X (the kernel's barrier).  trees: the scenario's forest sorted
// by x (ntree x DAT_TREE_STRIDE; ntree = 0: no forest).  In / out: the controller's warm state lamF, lamM (3n) and
// prev (n x 9).  Out: f_des (3n), err_seq (max_iter + 1, the residuals of the passes that did not stop), the
// agents' last QP status (n) and the IPM iterations of the slowest agent QP.  Returns the pass count.
int hs_dd_step(const double* prm, int n, const double* st, const double* acc, const double* trees, int ntree,
               double res_tol, int max_iter, double qp_tol, double* lamF, double* lamM, double* prev, double* f_des,
               double* err_seq, int* qstatus, int* ipmx) {
  const int N6 = 6 * n;
  std::vector<double> Hbuf((size_t)N6 * N6 + 2), Rts(9 * n), X(9 * n), E(6 * n), wrec((size_t)n * WREC_SIZE, 0.0);
  std::vector<double> best((size_t)n * best_size(1));
  double* Hinv = Hbuf.data() + (((size_t)Hbuf.data() & 15) ? 1 : 0);  // 16-byte aligned (dd_dual_ascent reads pairs)
  hs_dd_setup(prm, n, st, Hinv);
  const double* Rl = st + DAT_S_RL(n);
  QPShared S;
  build_shared(S, prm, n, st, acc, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, false);
  std::vector<QPLane<1>> P(n);
  std::vector<EnvRows> Ev(n);
  int nr = NBASE;
  for (int i = 0; i < n; ++i) {
    make_Rt(prm + DAT_P_RCOM(n) + 3 * i, Rl, Rts.data() + 9 * i);
    for (int c = 0; c < 9; ++c) X[9 * i + c] = prev[9 * i + c];  // the controller's current (f, F, M)
    qstatus[i] = ST_OPTIMAL;
    lane_dd_static(P[i], prm, i);
    if (ntree > 0) {  // k_dd<true>
      double lhs[DAT_NENV][3], rhs[DAT_NENV];
      unsigned emask;
      env_rows(prm, n, st, trees, ntree, i, prm[DAT_P_AENVD], &emask, lhs, rhs);
      set_env_rows(P[i], Ev[i], S, emask, lhs, rhs);
    }
    nr = nr > rows_needed(P[i].emask) ? nr : rows_needed(P[i].emask);
  }
  int iter = 0;
  bool lng = false;  // the long-chain rule (dd_long_chain)
  *ipmx = 0;
  for (;;) {
    for (int i = 0; i < n; ++i) {
      double c9[9], y[1][3], w[6];
      dd_prices(prm, n, i, lamF, lamM, Rl, c9);
      set_dd_price(P[i], prm, n, i, c9);
      const IPMOut o = ipm_solve_rows<MODE_DD, 1, IPM_FAST, true>(
          nr, PlainRef<QPShared>{&S}, EnvPlain{&Ev[i]}, RtPtr{Rts.data() + 9 * i}, P[i], prm + DAT_P_FEQ(n) + 3 * i, y,
          w, best.data() + (size_t)i * best_size(1), 50, dd_qp_tol(lng, qp_tol), wrec.data() + (size_t)i * WREC_SIZE,
          dd_warm_start(iter, lng));
      diag(o);
      *ipmx = *ipmx > o.iters ? *ipmx : o.iters;
      qstatus[i] = o.status;
      dd_take_solve(o.status, y[0], w, prm, n, i, X.data(), prev + 9 * i);
    }
    for (int c = 0; c < 9 * n; ++c) X[c] = prev[c];
    ++iter;
    for (int i = 0; i < n; ++i) dd_consensus_error(X.data(), Rts.data(), 9, n, i, E.data() + 6 * i);
    const double res = dd_pass_residual(E.data(), 6, n);
    if (dd_stop(res, res_tol, iter, max_iter)) break;
    err_seq[iter - 1] = res;
    lng = lng || dd_long_chain(iter, res);
    for (int i = 0; i < n; ++i)
      dd_dual_ascent(Hinv + (size_t)(6 * i) * N6, N6, E.data(), 6, n, lamF + 3 * i, lamM + 3 * i);
  }
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) f_des[3 * i + c] = X[9 * i + c];
  return iter;
}

// One C-ADMM control step of one scenario: cadmm_host_step (dat_cadmm_host.hpp).  The env rows come from the
// scenario's forest sorted by x (trees, ntree x 3; no rows pointer), or from the caller's compacted rows (row_lhs
// n x DAT_NENV x 3, row_rhs n x DAT_NENV, nrow n).  cfgd: res_tol, rho0, tau, rho_max, qp_tol; cfgi: max_iter,
// use_total_res, tail_prev, tail_pass.  In / out: the warm state cf, fbar, lam and *iters (the previous step's pass
// count in, this step's out).  Out: f_des, err_seq (max_iter + 1), qstatus (n) and what the observer counted --
// counts: solves, IPM iterations, redone solves, warm-started solves, loose accepts beyond Clarabel's 1e-8; per pass
// (max_iter + 1 each) the slowest solve's IPM iterations and the agents (bit i) warm-started and redone.
int hs_cadmm_step(const double* prm, int n, const double* st, const double* acc, const double* trees, int ntree,
                  const double* row_lhs, const double* row_rhs, const int* nrow, const double* cfgd, const int* cfgi,
                  double* cf, double* fbar, double* lam, int* iters, double* f_des, double* err_seq, int* qstatus,
                  long long* counts, int* pass_ipmx, int* pass_warm, int* pass_redone) {
  if (n < 3 || n > CADMM_HOST_NMAX) return -1;
  CadmmStepCfg cfg;
  cfg.res_tol = cfgd[0]; cfg.rho0 = cfgd[1]; cfg.tau = cfgd[2]; cfg.rho_max = cfgd[3]; cfg.qp_tol = cfgd[4];
  cfg.max_iter = cfgi[0]; cfg.use_total_res = cfgi[1]; cfg.tail_prev = cfgi[2]; cfg.tail_pass = cfgi[3];
  CadmmEnvSlots env[CADMM_HOST_NMAX];
  if (row_lhs) {
    for (int i = 0; i < n; ++i) {
      if (nrow[i] < 0 || nrow[i] > DAT_NENV) return -1;
      cadmm_env_of_rows(row_lhs + (size_t)i * DAT_NENV * 3, row_rhs + (size_t)i * DAT_NENV, nrow[i], env[i]);
    }
  } else {
    cadmm_env_of_trees(prm, n, st, trees, ntree, env);
  }
  for (int k = 0; k < 5; ++k) counts[k] = 0;
  for (int k = 0; k <= cfg.max_iter; ++k) pass_ipmx[k] = pass_warm[k] = pass_redone[k] = 0;
  cadmm_host_step(prm, n, st, acc, cfg, env, cf, fbar, lam, iters, f_des, err_seq, qstatus,
                  [&](int pass, int i, const QPLane<1>&, const IPMOut& o, bool warm) {
                    ++counts[0];
                    counts[1] += o.iters;
                    // (a warm solve's first attempt is the robust one, whose IPMOut::stiff means stiff rows)
                    const bool redone = o.stiff && !warm;
                    counts[2] += redone;
                    counts[3] += warm;
                    counts[4] += o.inband && o.merit > IPM_CLARABEL_TOL;
                    if (o.iters > pass_ipmx[pass]) pass_ipmx[pass] = o.iters;
                    pass_warm[pass] |= (warm ? 1 : 0) << i;
                    pass_redone[pass] |= (redone ? 1 : 0) << i;
                    diag(o);
                  });
  return 0;
}

int hs_qp_cent(const double* prm, int n, const double* st, const double* acc, const double* env_lhs,
               const double* env_rhs, int nenv, double* f_out, int* iters) {
  if (nenv > DAT_NENV) return -1;
  if (n == 3) return cent_nb_<3>(prm, st, acc, env_lhs, env_rhs, nenv, f_out, iters);
  if (n == 6) return cent_nb_<6>(prm, st, acc, env_lhs, env_rhs, nenv, f_out, iters);
  return -1;
}

int hs_env_rows(const double* prm, int n, const double* st, const double* trees, int ntree, int agent,
                double alpha, double* lhs, double* rhs, int* collision, double* min_dist) {
  double L[DAT_NENV][3], R[DAT_NENV];
  unsigned mask;
  EnvOut e = env_rows(prm, n, st, trees, ntree, agent, alpha, &mask, L, R);
  *collision = e.collision;
  *min_dist = e.min_env_dist;
  int k = 0;
  for (int j = 0; j < DAT_NENV; ++j) {
    if (!((mask >> j) & 1u)) continue;
    for (int c = 0; c < 3; ++c) lhs[3 * k + c] = L[j][c];
    rhs[k] = R[j];
    ++k;
  }
  return k;
}

void hs_sim_step(const double* prm, int n, double* st, int* counter, const double* fdes, double dt) {
  sim_step<16>(prm, n, st, counter, fdes, dt);
}

void hs_sim_step_ll(const double* prm, int n, double* st, int* counter, const double* fdes, double dt, int kind) {
  sim_step<16>(prm, n, st, counter, fdes, dt, kind);
}

void hs_rp_step(const double* prm, int n, double* st, int* counter, const double* f, double dt) {
  rp_step(prm, n, st, counter, f, dt);
}

void hs_ll_control(const double* R, const double* w, const double* J, const double* fdes, double* f, double* M) {
  ll_control_agent(R, w, J, fdes, f, M);
}

void hs_ll_control_kind(const double* R, const double* w, const double* J, const double* fdes, double* f, double* M,
                        int kind) {
  ll_control_agent(R, w, J, fdes, f, M, kind);
}

void hs_desired_accel(const double* st, int n, const double* mountain, double x_offset, double* acc) {
  desired_accel_forest(st, n, mountain, x_offset, acc);
}
}
