// dat_dd_step.hpp -- the lane-level rules of the dual-decomposition (DD) control step (control/rqp_dd.py:513-555,
// 642-693, 695-752), each stated once for every build that runs the step: the GPU kernels (k_dd_setup, dat_k_dd.hip;
// k_dd, dat_dd_drain.hpp) and the test-only host build (tests/hostsim).  A GPU lane calls them for its agent i (or its element of a
// matrix) between the kernels' barriers; a host build calls them in a loop.  Every floating-point expression
// stands whole inside one function: with -ffp-contract=on (multiply-adds fused within an expression only) an
// inlined copy computes the same bits at every call site.
#pragma once

#include "dat_qp.hpp"

namespace dat {

// ------------------------------------------------------------------ the warm rule and the drain key
// DD warm start: from DD pass DD_WARM_PASS of a step on, the agent QPs start from the previous pass's iterate (a
// long DD chain -- C3's slowest scenario runs the reference's cap of 100 passes at every step, the step's
// critical path; ordinary steps take ~4 passes and never reach it).  Its agent QP differs from the previous pass's
// only in the prices.  From pass 1 on it cut C3 further but left the n = 3 golden DD error sequence (25 fixed
// passes) 3e-4 off (bound 1e-4): a warm start lands elsewhere in a weakly convex QP's near-flat minimiser set than
// the reference's cold solve.  Same-call A/B (C3, ms per step): 21.7 -> 13.4 with DD_WS_MU 1e-3 (1e-2: 14.3);
// every DD parity test green (golden sequences, the DD hard stretch, the 100 s loop to the same horizon).  (The
// round-5 DD ran every pass cold; the build option that kept it for A/B builds went with this header.)
constexpr int DD_WARM_PASS = 30;
// The long-chain rule.  A cold agent-QP solve stops on the central path at a gap of 3-8e-10 (the first iterate under
// 10 tol), the same point pass after pass: its offset from the minimiser (the QPs are strongly convex only through
// the 1e-6 regularisation in some directions) is constant and the dual ascent absorbs it.  A warm solve stops
// elsewhere, so the first warm pass moved the residual by up to 4.5e-4 relative against the oracle's cold 1e-11
// solves (n = 8, a 44-pass step; the all-cold step 3e-5), beyond the oracle's own sensitivity (tests/_dd_long.py).
// A chain that is still DD_LONG_RES from consensus after DD_LONG_PASS passes is a long one (ordinary steps stop
// after ~4): from then on its agent QPs, cold and warm alike, are solved DD_LONG_TOL times tighter, which makes both
// offsets ten times smaller where the residual is still large, and only such a chain starts warm.  Host step,
// ref_dd_long.npz: IPM iterations per solve 10.4 -> 10.8 cold, 5.5 -> 5.9 warm.
constexpr int DD_LONG_PASS = 6;
constexpr double DD_LONG_RES = 0.5, DD_LONG_TOL = 0.1;
// after `iter` passes with residual res: the chain is a long one from here on
DAT_HD bool dd_long_chain(int iter, double res) { return iter == DD_LONG_PASS && res >= DD_LONG_RES; }
DAT_HD double dd_qp_tol(bool lng, double tol) { return lng ? fmax(DD_LONG_TOL * tol, 1e-12) : tol; }
DAT_HD bool dd_warm_pass(int iter) { return iter >= DD_WARM_PASS; }
// the agent QPs of pass `iter` start warm: a warm pass of a long chain
DAT_HD bool dd_warm_start(int iter, bool lng) { return lng && dd_warm_pass(iter); }
// The drain-order key's bin of a step's slowest agent QP (k_dd_key).  DD agent QPs run the conservative IPM start
// (9-10 iterations on average): bins <= 8, 9-10, 11-13, >= 14.
DAT_HD int dd_ipm_bin(int it) { return it <= 8 ? 0 : it <= 10 ? 1 : it <= 13 ? 2 : 3; }

// ------------------------------------------------------------------ Q_i and its inverse
// Q_i: strong_convexity_matrix (control/rqp_dd.py:513-555), 9x9 in (f_i, F_i, M_i)
DAT_HD void dd_strong_convexity(const double* prm, int n, const double* st, int i, double* Q) {
  const double kf = prm[DAT_P_KFD], km = prm[DAT_P_KMD], kfeq = prm[DAT_P_KFEQ];
  const double leader = (i == 0) ? 1.0 : 0.0;
  const double mT = prm[DAT_P_MT];
  const double* Rl = st + DAT_S_RL(n);
  double Rt[9], Xh[9], RX[9], Bv[9];
  make_Rt(prm + DAT_P_RCOM(n) + 3 * i, Rl, Rt);
  skew3(prm + DAT_P_XCOM, Xh);
  mm3(Rl, Xh, RX);
  mm3(RX, prm + DAT_P_JTI, Bv);  // Rl hat(x_com) JT^-1
  for (int k = 0; k < 81; ++k) Q[k] = 0.0;
  for (int k = 0; k < 9; ++k) Q[10 * k] = 1e-6;
  auto acc = [&](const double* T /*3x9*/, double wgt) {
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) Q[9 * r + c] += 2.0 * wgt * (T[r] * T[c] + T[9 + r] * T[9 + c] + T[18 + r] * T[18 + c]);
  };
  double T[27];
  for (int k = 0; k < 27; ++k) T[k] = 0.0;
  for (int r = 0; r < 3; ++r) T[9 * r + r] = 1.0;          // [I 0 0]
  acc(T, kfeq);
  for (int r = 0; r < 3; ++r) T[9 * r + 3 + r] = 1.0;      // [I I 0]
  acc(T, kf);
  for (int k = 0; k < 27; ++k) T[k] = 0.0;                 // [Rt 0 I]
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[9 * r + c] = Rt[3 * r + c];
    T[9 * r + 6 + r] = 1.0;
  }
  acc(T, km);
  if (leader != 0.0) {
    const double* JTi = prm + DAT_P_JTI;
    double JR[9], BR[9];
    mm3(JTi, Rt, JR);
    mm3(Bv, Rt, BR);
    for (int k = 0; k < 27; ++k) T[k] = 0.0;               // [JT^-1 Rt, 0, JT^-1]
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) { T[9 * r + c] = JR[3 * r + c]; T[9 * r + 6 + c] = JTi[3 * r + c]; }
    acc(T, leader);
    for (int k = 0; k < 27; ++k) T[k] = 0.0;               // [I/mT + Bv Rt, I/mT, Bv]
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        T[9 * r + c] = BR[3 * r + c] + (r == c ? 1.0 / mT : 0.0);
        T[9 * r + 3 + c] = (r == c ? 1.0 / mT : 0.0);
        T[9 * r + 6 + c] = Bv[3 * r + c];
      }
    acc(T, leader);
  }
}
// Q_i^-1 by Gauss-Jordan with partial pivoting (np.linalg.inv) on A = [Q_i | I] (9 x 18, row-major), in the steps
// of the serial elimination: at step k the pivot row, the row exchange, the copy of column k before the update
// (colk, 9), the update of every column c, and at the end the symmetrised right half.  The GPU spreads the
// elements c of a step over lanes; the host runs them in a loop.
DAT_HD void dd_qinv_augment(const double* Q, double* A) {
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 18; ++c) A[18 * r + c] = c < 9 ? Q[9 * r + c] : (c - 9 == r ? 1.0 : 0.0);
}
DAT_HD int dd_qinv_pivot_row(const double* A, int k) {
  int p = k;
  for (int r = k + 1; r < 9; ++r)
    if (fabs(A[18 * r + k]) > fabs(A[18 * p + k])) p = r;
  return p;
}
DAT_HD void dd_qinv_exchange(double* A, int k, int p, int c) {
  if (p != k) { double t = A[18 * k + c]; A[18 * k + c] = A[18 * p + c]; A[18 * p + c] = t; }
}
DAT_HD void dd_qinv_update_col(double* A, const double* colk, int k, int c) {
  const double inv = 1.0 / colk[k];
  const double hk = A[18 * k + c] * inv;
  A[18 * k + c] = hk;
  for (int r = 0; r < 9; ++r)
    if (r != k) A[18 * r + c] -= colk[r] * hk;
}
DAT_HD double dd_qinv_sym(const double* A, int r, int c) { return 0.5 * (A[18 * r + 9 + c] + A[18 * c + 9 + r]); }

// ------------------------------------------------------------------ H = A blkdiag(Q_j^-1) A' and its inverse
// Row r of A restricted to agent block j (control/rqp_dd.py:642-655), 9 entries on (f_j, F_j, M_j):
//   j == agent(r): the unit vector e_{3 + comp};  j != agent(r): -e_comp (comp < 3) or -Rt_j[comp-3, :] on f_j.
// Rt_j: agent j's U-map (9, row-major).  Every index is compile-time after unrolling, so v stays in registers.
DAT_HD void dd_arow(int r, int j, const double* Rt_j, double* v) {
  const int ag = r / 6, comp = r % 6;
  const double* rt = Rt_j + 3 * (comp >= 3 ? comp - 3 : 0);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    double x = 0.0;
    if (j == ag) x = (k == 3 + comp) ? 1.0 : 0.0;
    else if (comp < 3) x = (k == comp) ? -1.0 : 0.0;
    else if (k < 3) x = -rt[k];
    v[k] = x;
  }
}
// One element H_rc: summed over blocks j, then over the support p of row r's block in increasing order, of
// A_rp (Q_j^-1 A_c)_p with (Q_j^-1 A_c)_p summed over q in increasing order.  Qi: n x 81 sym(Q_j^-1), Rts: n x 9.
DAT_HD double dd_h_element(const double* Qi, const double* Rts, int n, int r, int c) {
  double s = 0.0;
  for (int j = 0; j < n; ++j) {
    double vr[9], vc[9];
    dd_arow(r, j, Rts + 9 * j, vr);
    dd_arow(c, j, Rts + 9 * j, vc);
    const double* Q = Qi + 81 * j;
#pragma unroll
    for (int p = 0; p < 9; ++p) {
      if (vr[p] == 0.0) continue;
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < 9; ++q) t += Q[9 * p + q] * vc[q];
      s += vr[p] * t;
    }
  }
  return s;
}
// H^-1 by Gauss-Jordan on [H | I] without pivoting (H is SPD): at step k, per element of a column,
// hk = h_kc / piv for the pivot row and h_rc -= f_r hk for the others (f: column k before the step).
DAT_HD double dd_hinv_scale(double h_kc, double piv) { return h_kc / piv; }
DAT_HD void dd_hinv_eliminate(double& h_rc, double f_r, double hk) { h_rc -= f_r * hk; }
// Column c of [H | I] (N rows, ld doubles apart) at step k
DAT_HD void dd_hinv_update_col(double* H, int ld, int N, const double* fac, double piv, int k, int c) {
  const double hk = dd_hinv_scale(H[ld * k + c], piv);
  H[ld * k + c] = hk;
  for (int r = 0; r < N; ++r)
    if (r != k) dd_hinv_eliminate(H[ld * r + c], fac[r], hk);
}

// ------------------------------------------------------------------ the pass
// Agent records of one scenario: X (n x 9, (f, F, M) of every agent), E (n records es doubles apart: the consensus
// error, 6 values each), Rts (n U-maps rt_stride doubles apart), lamF / lamM (3n, agent-major).
// The prices c9 = (c_fi, c_Fi, c_Mi) of agent i (control/rqp_dd.py:718-722)
DAT_HD void dd_prices(const double* prm, int n, int i, const double* lF, const double* lM, const double* Rl,
                      double* c9) {
  double sF[3] = {0, 0, 0}, sM[3] = {0, 0, 0};
  for (int k = 0; k < n; ++k)
    for (int c = 0; c < 3; ++c) { sF[c] += lF[3 * k + c]; sM[c] += lM[3 * k + c]; }
  double dm[3], rxd[3], Rr[3];
  for (int c = 0; c < 3; ++c) dm[c] = sM[c] - lM[3 * i + c];
  cross3(prm + DAT_P_RCOM(n) + 3 * i, dm, rxd);
  mv3(Rl, rxd, Rr);
  for (int c = 0; c < 3; ++c) {
    c9[c] = -(sF[c] - lF[3 * i + c]) + Rr[c];
    c9[3 + c] = lF[3 * i + c];
    c9[6 + c] = lM[3 * i + c];
  }
}
// What a solve's status does to the agent's held (f, F, M) (RQPDualSolver.solve): OPTIMAL takes (y, w), a solver
// exception the fallback (control/rqp_dd.py:484-489), anything else holds the previous value (:491-496).
// Quirk a15: the controller's f aliases solver 0's f_eq (control/rqp_dd.py:629, written in place at :725), so
// agent 0's fallback sums the controller's current forces (X: every agent's f before this pass's writes); the
// other agents sum their own f_eq.
DAT_HD void dd_take_solve(int status, const double* y, const double* w, const double* prm, int n, int i,
                          const double* X, double* held) {
  if (status == ST_OPTIMAL) {
    for (int c = 0; c < 3; ++c) held[c] = y[c];
    for (int c = 0; c < 6; ++c) held[3 + c] = w[c];
  } else if (status == ST_FAILED) {
    const double* feq = prm + DAT_P_FEQ(n);
    double s3[3] = {0, 0, 0};
    for (int k = 0; k < n; ++k)
      for (int c = 0; c < 3; ++c) s3[c] += (i == 0) ? X[k * 9 + c] : feq[3 * k + c];
    dd_fallback(prm, n, i, s3, held);
  }
}
// Agent i's consensus error (control/rqp_dd.py:659-676): E_F,i = F_i - sum_{k != i} f_k, E_M,i likewise with the
// moments of f_k (Ei: F (3), then M (3))
DAT_HD void dd_consensus_error(const double* X, const double* Rts, int rt_stride, int n, int i, double* Ei) {
  const double* myX = X + i * 9;
  double sf[3] = {0, 0, 0}, sm[3] = {0, 0, 0};
  for (int k = 0; k < n; ++k) {
    if (k == i) continue;
    const double* fk = X + k * 9;
    double m3[3];
    mv3(Rts + rt_stride * k, fk, m3);
    for (int c = 0; c < 3; ++c) { sf[c] += fk[c]; sm[c] += m3[c]; }
  }
  for (int c = 0; c < 3; ++c) {
    Ei[c] = myX[3 + c] - sf[c];
    Ei[3 + c] = myX[6 + c] - sm[c];
  }
}
// The pass residual: the largest of the six column sums of |E| (the matrix 1-norm of the n x 6 error), and the
// stop test after `iter` passes
DAT_HD double dd_pass_residual(const double* E, int es, int n) {
  double res = 0.0;
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += fabs(E[k * es + r]);
    res = fmax(res, s);
  }
  return res;
}
DAT_HD bool dd_stop(double res, double res_tol, int iter, int max_iter) { return (res < res_tol) || (iter > max_iter); }
// Dual ascent of agent i: lambda += H^-1 (A x) (control/rqp_dd.py:678-693), rows 6i..6i+5 (Hi: row 6i of H^-1,
// rows N6 doubles apart, 16-byte aligned).  The six rows are read agent block by agent block (18 16-byte loads in
// flight per block, rows and blocks 48-byte aligned), each row's sum kept in the original order c = 0 .. 6n-1.
DAT_HD void dd_dual_ascent(const double* Hi, int N6, const double* E, int es, int n, double* lFi, double* lMi) {
  double stp[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n; ++k) {
    dat_d2 h[6][3];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int j = 0; j < 3; ++j) h[r][j] = *(const dat_d2*)(Hi + (size_t)r * N6 + 6 * k + 2 * j);
    const double* e = E + k * es;
    double ev[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) ev[j] = e[j];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        stp[r] += h[r][j].x * ev[2 * j];
        stp[r] += h[r][j].y * ev[2 * j + 1];
      }
  }
  for (int c = 0; c < 3; ++c) {
    lFi[c] += stp[c];
    lMi[c] += stp[3 + c];
  }
}

}  // namespace dat
