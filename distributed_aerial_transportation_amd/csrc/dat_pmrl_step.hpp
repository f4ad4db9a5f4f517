// dat_pmrl_step.hpp -- the rules of one step of the point-mass rigid-link system, each stated once.
//
// PMRLDynamics (system/point_mass_rigid_link.py:135-254): n point-mass robots carry the rigid payload on rigid
// links.  State: link directions q_i on S^2 with tangent rates dq_i, and the payload (xl, vl, Rl, wl).  Input: the
// thrusts f_i (ground frame).  Equations of motion, with x_i = xl + L_i q_i + Rl r_i:
//     m_i x_i'' = f_i - m_i g e3 - T_i q_i,     ml dvl = sum_i T_i q_i - ml g e3,
//     Jl dwl + wl x Jl wl = sum_i hat(r_i) T_i Rl' q_i,     q_i . ddq_i = -|dq_i|^2.
//
// The link tensions T.  The reference solves the n x n SPD system (:176-198)
//     (diag(1/m) + q'q / ml + (U c)'(U c)) T = rhs,   c_i = r_i x Rl' q_i,  U'U = Jl^-1,
// by a dense Cholesky.  Its matrix is M^-1 + G'G with M = diag(m) and the 6 x n matrix G = [q / sqrt(ml); U c]
// (columns g_i), so by Woodbury, with y = M rhs,
//     S z = G y,   S = I_6 + G M G' = I_6 + sum_i m_i g_i g_i',   T_i = y_i - m_i g_i . z :
// one 6 x 6 SPD system whose size does not depend on n and whose eigenvalues are >= 1 (its Cholesky cannot break
// down).  And G T = z: the payload's force sum q T = sqrt(ml) z[0:3] and Jl^-1 c T = U' z[3:6] follow from z, no
// second sum over the links.  
//
// The pieces below are what a GPU lane (k_pmrl_rollout / k_pmrl_forward, dat_k_step.hip: one lane per link, (m_i, y_i,
// g_i) through LDS) and the serial host forms at the end of this file (pmrl_forward, pmrl_step: the test builds)
// both run.  Every floating-point expression stands whole inside one piece (the rule of dat_cadmm_step.hpp); the
// sums over the links run in the order i = 0 .. n-1 in both.
#pragma once

#include "dat_core.hpp"

namespace dat {

// what every link of a scenario shares (:170-174): cor_acc = Jl^-1 (wl x Jl wl), cor_mat = Rl (hat(wl)^2 - hat(cor_acc))
struct PmrlPayload {
  double cor_acc[3] = {0, 0, 0}, cor_mat[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};
DAT_HD void pmrl_payload_terms(const double* prm, const double* Rl, const double* wl, PmrlPayload& p) {
  double Jw[3], wJw[3], W[9], W2[9], C[9], D[9];
  mv3(prm + DAT_P_JT, wl, Jw);
  cross3(wl, Jw, wJw);
  mv3(prm + DAT_P_JTI, wJw, p.cor_acc);
  skew3(wl, W);
  mm3(W, W, W2);
  skew3(p.cor_acc, C);
  for (int k = 0; k < 9; ++k) D[k] = W2[k] - C[k];
  mm3(Rl, D, p.cor_mat);
}

// one link's terms: add = f - cor_mat (m r) (:175); y = m rhs = add . q + m L |dq|^2 (:176-179 before the division
// by m); g = (q / sqrt(ml), U (r x Rl' q)), its column of G (:180-183)
struct PmrlLink {
  double add[3] = {0, 0, 0}, y = 0.0, g[6] = {0, 0, 0, 0, 0, 0};
};
DAT_HD void pmrl_link_terms(const double* prm, int n, int i, const PmrlPayload& p, const double* Rl, const double* q,
                            const double* dq, const double* f, PmrlLink& k) {
  const double m = prm[DAT_P_PM_M(n) + i], L = prm[DAT_P_PM_L(n) + i];
  const double* r = prm + DAT_P_R(n) + 3 * i;
  const double* U = prm + DAT_P_PM_U(n);  // upper factor, row-major: the entries below the diagonal are zero
  const double mr[3] = {m * r[0], m * r[1], m * r[2]};
  double cm[3], qb[3], c[3];
  mv3(p.cor_mat, mr, cm);
  for (int a = 0; a < 3; ++a) k.add[a] = f[a] - cm[a];
  k.y = dot3(k.add, q) + m * L * dot3(dq, dq);
  const double sml = sqrt(prm[DAT_P_MT]);
  for (int a = 0; a < 3; ++a) k.g[a] = q[a] / sml;
  mtv3(Rl, q, qb);
  cross3(r, qb, c);
  k.g[3] = U[0] * c[0] + U[1] * c[1] + U[2] * c[2];
  k.g[4] = U[4] * c[1] + U[5] * c[2];
  k.g[5] = U[8] * c[2];
}

// the reduced system (S packed upper, sp6): S = I_6, G y = 0, then one link after the other, i = 0 .. n-1
DAT_HD void pmrl_system_clear(double* S, double* Gy) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    Gy[r] = 0.0;
#pragma unroll
    for (int c = r; c < 6; ++c) S[sp6(r, c)] = (r == c) ? 1.0 : 0.0;
  }
}
DAT_HD void pmrl_system_add(double* S, double* Gy, double m, double y, const double* g) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double mg = m * g[r];
    Gy[r] += g[r] * y;
#pragma unroll
    for (int c = r; c < 6; ++c) S[sp6(r, c)] += mg * g[c];
  }
}
// z = S^-1 (G y), in place, by the 6 x 6 Cholesky (S >= I: every pivot is >= 1)
DAT_HD void pmrl_solve6(const double* S, double* z) {
  double Lf[21];
  chol6(S, Lf);
  chol6_solve(Lf, z);
}
// T_i = y_i - m_i g_i . z
DAT_HD double pmrl_tension(double m, double y, const double* g, const double* z) {
  return y - m * (g[0] * z[0] + g[1] * z[1] + g[2] * z[2] + g[3] * z[3] + g[4] * z[4] + g[5] * z[5]);
}

// the payload's accelerations from z = G T (:199-200, 206-207): qT = sum q_i T_i = sqrt(ml) z[0:3],
// aT = Jl^-1 sum c_i T_i = U' z[3:6]; dvl = qT / ml - g e3, dwl = aT - cor_acc
struct PmrlSums {
  double qT[3] = {0, 0, 0}, aT[3] = {0, 0, 0};
};
DAT_HD void pmrl_payload_accel(const double* prm, int n, const PmrlPayload& p, const double* z, PmrlSums& s,
                               double* dvl, double* dwl) {
  const double ml = prm[DAT_P_MT];
  const double sml = sqrt(ml);
  const double* U = prm + DAT_P_PM_U(n);
  for (int a = 0; a < 3; ++a) s.qT[a] = sml * z[a];
  s.aT[0] = U[0] * z[3];
  s.aT[1] = U[1] * z[3] + U[4] * z[4];
  s.aT[2] = U[2] * z[3] + U[5] * z[4] + U[8] * z[5];
  for (int a = 0; a < 3; ++a) {
    dvl[a] = s.qT[a] / ml;
    dwl[a] = s.aT[a] - p.cor_acc[a];
  }
  dvl[2] -= DAT_GRAVITY;
}
// one link's acceleration (:201-205): ddq = (add - q T) / (m L) - qT / (ml L) - Rl hat(aT) r / L
DAT_HD void pmrl_link_accel(const double* prm, int n, int i, const double* Rl, const PmrlLink& k, const double* q,
                            double T, const PmrlSums& s, double* ddq) {
  const double m = prm[DAT_P_PM_M(n) + i], L = prm[DAT_P_PM_L(n) + i], ml = prm[DAT_P_MT];
  const double* r = prm + DAT_P_R(n) + 3 * i;
  double ar[3], Ra[3];
  cross3(s.aT, r, ar);
  mv3(Rl, ar, Ra);
  for (int a = 0; a < 3; ++a) ddq[a] = (k.add[a] - q[a] * T) / (m * L) - s.qT[a] / (ml * L) - Ra[a] / L;
}
// a link's integration with its projection (:101-105, 122-124): q on S^2, then dq on the tangent space of the new q
DAT_HD void pmrl_integrate_link(double* q, double* dq, const double* ddq, double dt) {
  for (int a = 0; a < 3; ++a) {
    q[a] = q[a] + dq[a] * dt + ddq[a] * (dt * dt) / 2.0;
    dq[a] = dq[a] + ddq[a] * dt;
  }
  const double nq = sqrt(dot3(q, q));
  for (int a = 0; a < 3; ++a) q[a] = q[a] / nq;
  const double qd = dot3(q, dq);
  for (int a = 0; a < 3; ++a) dq[a] = dq[a] - q[a] * qd;
}
// the payload's integration (:125-132): integrate_lin, integrate_rot, and polar3 on Rl alone when it is due
DAT_HD void pmrl_integrate_payload(double* xl, double* vl, double* Rl, double* wl, const double* dvl,
                                   const double* dwl, double dt, int* counter) {
  integrate_lin(xl, vl, dvl, dt);
  integrate_rot(Rl, wl, dwl, dt);
  if (projection_due(counter)) polar3(Rl);
}

// ---- the serial forms: the links one after the other (host builds; the kernels run the same pieces per lane) -------
// PMRLDynamics.forward_dynamics (:156-208) at the state block st with the thrusts f (3n, agent-major):
// ddq (3n, agent-major), dvl (3), dwl (3), T (n)
template <int NMAX>
DAT_HD void pmrl_forward(const double* prm, int n, const double* st, const double* f, double* ddq, double* dvl,
                         double* dwl, double* T) {
  const double* Rl = st + DAT_S_RL(n);
  PmrlPayload p;
  pmrl_payload_terms(prm, Rl, st + DAT_S_WL(n), p);
  PmrlLink lk[NMAX];
  double S[21], z[6];
  pmrl_system_clear(S, z);
  for (int i = 0; i < n; ++i) {
    pmrl_link_terms(prm, n, i, p, Rl, st + DAT_S_Q(n) + 3 * i, st + DAT_S_DQ(n) + 3 * i, f + 3 * i, lk[i]);
    pmrl_system_add(S, z, prm[DAT_P_PM_M(n) + i], lk[i].y, lk[i].g);
  }
  pmrl_solve6(S, z);
  PmrlSums s;
  pmrl_payload_accel(prm, n, p, z, s, dvl, dwl);
  for (int i = 0; i < n; ++i) {
    T[i] = pmrl_tension(prm[DAT_P_PM_M(n) + i], lk[i].y, lk[i].g, z);
    pmrl_link_accel(prm, n, i, Rl, lk[i], st + DAT_S_Q(n) + 3 * i, T[i], s, ddq + 3 * i);
  }
}
// PMRLDynamics.integrate (:251-254): one step of dt under the thrusts f; counter: steps since the last projection
template <int NMAX>
DAT_HD void pmrl_step(const double* prm, int n, double* st, int* counter, const double* f, double dt) {
  double ddq[3 * NMAX], dvl[3], dwl[3], T[NMAX];
  pmrl_forward<NMAX>(prm, n, st, f, ddq, dvl, dwl, T);
  for (int i = 0; i < n; ++i) pmrl_integrate_link(st + DAT_S_Q(n) + 3 * i, st + DAT_S_DQ(n) + 3 * i, ddq + 3 * i, dt);
  pmrl_integrate_payload(st + DAT_S_XL(n), st + DAT_S_VL(n), st + DAT_S_RL(n), st + DAT_S_WL(n), dvl, dwl, dt,
                         counter);
}

}  // namespace dat
