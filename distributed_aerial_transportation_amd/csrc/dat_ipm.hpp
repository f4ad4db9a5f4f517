// dat_ipm.hpp -- the interior-point solver of the reduced agent QP (per-lane fp64 device code): the cone
// algebra, the row stores, the solver's stateless pieces (the cone map G, the linear maps of u, the row access),
// ipm_attempt and the solves built on it (ipm_solve, ipm_solve_rows).  The QP's data and the constants:
// dat_qp.hpp, which includes this file at its end and is the include everyone uses.
#pragma once

#include "dat_qp.hpp"

namespace dat {

// =====================================================================================
// interior-point method on the reduced problem
// =====================================================================================
// Per cone block: slack/dual layout [fz | soc1 (4) | soc2 (4)] (9 entries),
//   s = h - G y,  G y = -(y2, sec y2, y0, y1, y2, 0, y0, y1, y2),  h = (-min_fz, 0,0,0,0, max_f, 0,0,0).
// Cone blocks use Nesterov-Todd scaling; the LP rows (u-slots) are carried unscaled (for the
// nonnegative orthant NT scaling is diagonal and the two forms are algebraically identical).
struct SocScale {
  double w0, w1, w2, w3, eta, ieta, k1;  // k1 = 1 / (1 + w0)
};

DAT_HD double soc_det(const double* v) {
  double n1 = sqrt(v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
  return (v[0] - n1) * (v[0] + n1);
}
DAT_HD bool soc_scaling(const double* s, const double* z, SocScale& S) {
  double ds = soc_det(s), dz = soc_det(z);
  if (!(ds > 0) || !(dz > 0)) return false;
  double sn = sqrt(ds), zn = sqrt(dz);
  double isn = frcp(sn), izn = frcp(zn);
  double s0 = s[0] * isn, s1 = s[1] * isn, s2 = s[2] * isn, s3 = s[3] * isn;
  double z0 = z[0] * izn, z1 = z[1] * izn, z2 = z[2] * izn, z3 = z[3] * izn;
  double g = sqrt(0.5 * (1.0 + s0 * z0 + s1 * z1 + s2 * z2 + s3 * z3));
  double ig = 0.5 * frcp(g);
  S.w0 = (s0 + z0) * ig;
  S.w1 = (s1 - z1) * ig;
  S.w2 = (s2 - z2) * ig;
  S.w3 = (s3 - z3) * ig;
  S.eta = sqrt(sn * izn);
  S.ieta = frcp(S.eta);
  S.k1 = frcp(1.0 + S.w0);
  return true;
}
// o = W v (inv = false) or W^-1 v (inv = true); W = eta H(w), W^-1 = H(Jw)/eta
DAT_HD void soc_apply(const SocScale& S, const double* v, double* o, bool inv) {
  const double sg = inv ? -1.0 : 1.0;
  const double w1 = sg * S.w1, w2 = sg * S.w2, w3 = sg * S.w3;
  const double wv = w1 * v[1] + w2 * v[2] + w3 * v[3];
  const double k = v[0] + wv * S.k1;
  const double sc = inv ? S.ieta : S.eta;
  const double o0 = S.w0 * v[0] + wv;
  o[1] = sc * (v[1] + k * w1);
  o[2] = sc * (v[2] + k * w2);
  o[3] = sc * (v[3] + k * w3);
  o[0] = sc * o0;
}
// x = lam \ y (inverse Jordan product) for a 4-dim SOC
DAT_HD void soc_jdiv(const double* l, const double* y, double* x) {
  double det = l[0] * l[0] - (l[1] * l[1] + l[2] * l[2] + l[3] * l[3]);
  double x0 = (l[0] * y[0] - (l[1] * y[1] + l[2] * y[2] + l[3] * y[3])) * frcp(det);
  double il0 = frcp(l[0]);
  x[0] = x0;
  x[1] = (y[1] - x0 * l[1]) * il0;
  x[2] = (y[2] - x0 * l[2]) * il0;
  x[3] = (y[3] - x0 * l[3]) * il0;
}
DAT_HD void soc_jprod(const double* a, const double* b, double* o) {
  double d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  o[1] = a[0] * b[1] + b[0] * a[1];
  o[2] = a[0] * b[2] + b[0] * a[2];
  o[3] = a[0] * b[3] + b[0] * a[3];
  o[0] = d;
}
// largest step a with x + a d in the SOC (1e300 if unbounded)
DAT_HD double soc_step(const double* x, const double* d) {
  double a = d[0] * d[0] - (d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
  double b = x[0] * d[0] - (x[1] * d[1] + x[2] * d[2] + x[3] * d[3]);
  double n1 = sqrt(x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
  double c = (x[0] - n1) * (x[0] + n1);
  double disc = b * b - a * c;
  if (a < 0.0 || (b < 0.0 && disc >= 0.0)) {
    double den = -b + sqrt(fmax(disc, 0.0));
    return den > 0.0 ? c * frcp(den) : 0.0;
  }
  return 1e300;
}

// Per-row IPM state (slack s_l, dual z_l, Newton row term zw_l of each row slot).  RowRegs keeps
// it in registers; RowLds in an LDS image over the 64 lanes of a wavefront: the (s_l, z_l) pair of
// slot l of lane j at doubles [l 128 + 2 j, +1] (one ds_read_b128 / ds_write_b128 per pair; a
// wavefront touches 1 KB of consecutive LDS), zw_l at [2 NR 64 + l 64 + j]; read and written through
// volatile pointers, so the rows cost no registers between uses.  Besides the rows, a store may hold
// NX auxiliary per-lane doubles at [(3 NR + k) 64 + j] (aux slots: the per-iteration quantities
// ipm_solve's AUXM mask moves out of the register file, see ipm_aux_doubles).
struct RowRegs {
  template <int NR, int NX = 0>
  struct Store {
    double s_[NR], z_[NR], w_[NR], x_[NX > 0 ? NX : 1];
    DAT_HD explicit Store(const RowRegs&) {}
    DAT_HD double& s(int l) { return s_[l]; }
    DAT_HD double& z(int l) { return z_[l]; }
    DAT_HD double& w(int l) { return w_[l]; }
    DAT_HD double& x(int k) { return x_[k]; }
    DAT_HD void sz(int l, double& sv, double& zv) { sv = s_[l]; zv = z_[l]; }
    DAT_HD void set_sz(int l, double sv, double zv) { s_[l] = sv; z_[l] = zv; }
  };
};
struct RowLds {
  double* base;
  int lane;
  template <int NR, int NX = 0>
  struct Store {
    DAT_LDS double* p;   // the lane's zw / aux column
    DAT_LDS double* pz;  // the lane's (s, z) pair column
    __device__ explicit Store(const RowLds& r)
        : p((DAT_LDS double*)(r.base + r.lane)), pz((DAT_LDS double*)(r.base + 2 * r.lane)) {}
    __device__ volatile DAT_LDS double& at(int k) { return ((volatile DAT_LDS double*)p)[k * 64]; }
    __device__ volatile DAT_LDS double& s(int l) { return ((volatile DAT_LDS double*)pz)[l * 128]; }
    __device__ volatile DAT_LDS double& z(int l) { return ((volatile DAT_LDS double*)pz)[l * 128 + 1]; }
    __device__ volatile DAT_LDS double& w(int l) { return at(2 * NR + l); }
    __device__ volatile DAT_LDS double& x(int k) { return at(3 * NR + k); }
    __device__ void sz(int l, double& sv, double& zv) {
      const dat_d2 v = ((volatile DAT_LDS dat_d2*)pz)[l * 64];
      sv = v.x;
      zv = v.y;
    }
    __device__ void set_sz(int l, double sv, double zv) {
      dat_d2 v;
      v.x = sv;
      v.y = zv;
      ((volatile DAT_LDS dat_d2*)pz)[l * 64] = v;
    }
  };
};
// Host model of RowLds (the same strided columns in ordinary memory): exercises the aux / row store
// code paths of ipm_solve in the host build (tests/hostsim).
struct RowMem {
  double* base;
  int lane;
  template <int NR, int NX = 0>
  struct Store {
    double* p;
    double* pz;
    DAT_HD explicit Store(const RowMem& r) : p(r.base + r.lane), pz(r.base + 2 * r.lane) {}
    DAT_HD double& at(int k) { return p[k * 64]; }
    DAT_HD double& s(int l) { return pz[l * 128]; }
    DAT_HD double& z(int l) { return pz[l * 128 + 1]; }
    DAT_HD double& w(int l) { return at(2 * NR + l); }
    DAT_HD double& x(int k) { return at(3 * NR + k); }
    DAT_HD void sz(int l, double& sv, double& zv) { sv = s(l); zv = z(l); }
    DAT_HD void set_sz(int l, double sv, double zv) { s(l) = sv; z(l) = zv; }
  };
};
// aux slots of ipm_solve (AUXM bits): SCAL the stopping-rule scales and best merits (4), RES the
// iteration's residuals r_y and R_f (3 NB + 6), LAM the scaled point lambda = W z (9 NB), DINV the
// cone blocks' QR factor of D (qr_cone) and 1 / d0 (7 NB)
constexpr unsigned AUX_SCAL = 1, AUX_RES = 2, AUX_LAM = 4, AUX_DINV = 8;
__host__ __device__ constexpr int ipm_aux_doubles(int NB, unsigned AUXM) {
  return ((AUXM & AUX_SCAL) ? 4 : 0) + ((AUXM & AUX_RES) ? 3 * NB + 6 : 0) + ((AUXM & AUX_LAM) ? 9 * NB : 0) +
         ((AUXM & AUX_DINV) ? 7 * NB : 0);
}
__host__ __device__ constexpr int row_lds_doubles(int NR, int NX = 0) { return (3 * NR + NX) * 64; }  // (s, z) pairs, zw, aux

// Phase profile (development builds only, -DDAT_PHASE_PROF): shader-clock cycles per phase of the
// IPM iteration, summed over wavefronts by the first active lane (tools/phase_prof.py).
#if defined(DAT_PHASE_PROF)
__device__ unsigned long long g_phase[16];
#endif
#if defined(DAT_ITER_HIST)
// IPM iteration histogram of the agent QPs (development builds, tools/iter_hist.py): [iters] solves
__device__ unsigned long long g_iter_hist[64];
#endif
#if defined(DAT_PHASE_PROF) && defined(__HIP_DEVICE_COMPILE__)
struct PhaseClock {
  unsigned long long t0;
  int cur;
  __device__ PhaseClock(int c) : t0(clock64()), cur(c) {}
  __device__ void to(int next) {
    const unsigned long long t = clock64();
    const unsigned long long act = __ballot(1);
    if ((int)__lane_id() == __ffsll((long long)act) - 1) atomicAdd(&g_phase[cur], t - t0);
    t0 = t;
    cur = next;
  }
};
#define DAT_PHASE_INIT(c) PhaseClock pclk_(c)
#define DAT_PHASE(c) pclk_.to(c)
#else
#define DAT_PHASE_INIT(c)
#define DAT_PHASE(c)
#endif

// Refinement statistics (host builds with -DDAT_IPM_STATS only, tools/ipm_stats.py): corrector solves,
// refinement passes run, passes skipped by the rounding-level test.
#if defined(DAT_IPM_STATS) && !defined(__HIP_DEVICE_COMPILE__)
inline long long g_ipm_stats[16];  // [0..2] refinement, [3 + why] non-converged exits, [10] in-band, [11] solves
inline long long g_ipm_hist[3][24];  // [first pass stopped at rounding | correction applied | 2nd pass][log10 max row z/s + 12]
inline double g_maxw;
#define DAT_STAT(k) (++g_ipm_stats[k])
#define DAT_STAT_W(w) (g_maxw = (w) > g_maxw ? (w) : g_maxw)
#define DAT_STAT_H(k)                                                                   \
  do {                                                                                  \
    int b_ = g_maxw > 0 ? (int)floor(log10(g_maxw)) + 12 : 0;                           \
    ++g_ipm_hist[k][b_ < 0 ? 0 : b_ > 23 ? 23 : b_];                                    \
  } while (0)
#else
#define DAT_STAT(k) ((void)0)
#define DAT_STAT_W(w) ((void)0)
#define DAT_STAT_H(k) ((void)0)
#endif

// Cone-block groups.  ipm_solve sums (max, min) its per-block quantities over the blocks a lane
// holds; a group policy extends those reductions over the W lanes of a lane group, so one QP's cone
// blocks can live on W lanes (the centralized QP: one agent's force per lane, dat_cent.hip).  The
// u-space algebra and the row slots are replicated on the group's lanes, so every lane must see
// bit-identical reduced values: the reductions are xor butterflies, whose pairwise sums are computed
// in both orders and IEEE addition / fmax / fmin are commutative.
struct NoGrp {  // one lane holds all blocks of its QP
  static constexpr bool on = false;
  DAT_HD bool act() const { return true; }
  DAT_HD int nblk(int NB) const { return NB; }
  DAT_HD double sum(double x) const { return x; }
  DAT_HD double max(double x) const { return x; }
  DAT_HD double min(double x) const { return x; }
};
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// x of the lane selected by DPP control CTRL (row-local: a group never reads another group's lanes)
template <int CTRL>
__device__ inline double dpp_d(double x) {
  const long long v = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v & 0xffffffffll), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
// W (4, 8 or 16) lanes, aligned to W: quad_perm xor 1, quad_perm xor 2, row_half_mirror (lane i <-> 7 - i),
// row_mirror (i <-> 15 - i).  Each step combines the lane's partial with its partner group's.
template <int W>
struct GrpDpp {
  static_assert(W == 4 || W == 8 || W == 16, "group width");
  static constexpr bool on = true;
  bool active;  // the lane holds a real block (phantom lanes k >= n contribute nothing)
  int n;        // blocks of the QP
  template <class F>
  __device__ double red(double x, F f) const {
    x = f(x, dpp_d<0xB1>(x));    // quad_perm [1, 0, 3, 2]
    x = f(x, dpp_d<0x4E>(x));    // quad_perm [2, 3, 0, 1]
    if (W >= 8) x = f(x, dpp_d<0x141>(x));   // row_half_mirror
    if (W >= 16) x = f(x, dpp_d<0x140>(x));  // row_mirror
    return x;
  }
  __device__ bool act() const { return active; }
  __device__ int nblk(int) const { return n; }
  __device__ double sum(double x) const { return red(active ? x : 0.0, [](double a, double b) { return a + b; }); }
  __device__ double max(double x) const { return red(active ? x : 0.0, [](double a, double b) { return fmax(a, b); }); }
  __device__ double min(double x) const { return red(active ? x : 1e300, [](double a, double b) { return fmin(a, b); }); }
};
#endif

struct IPMOut {
  int status;
  int iters;
  int inband;     // OPTIMAL through the best in-band iterate of a stalled solve (not converged to tol)
  double merit;   // scaled max(primal residual, dual residual, gap) of the returned iterate
  int why;        // exit: 0 converged, 1 non-finite residuals, 2 divergence / max_iter, 3 cone scaling,
                  // 4 cone block D, 5 Cholesky of M, 6 Cholesky of N
  int refs;       // refinement passes run (residual evaluations of the linearised system)
  int corrs;      // refinement corrections applied (core solves)
  int stiff;      // IPM_ROBUST: stiff rows solved in augmented form in some iteration; IPM_FAST_REDO: redone robustly
  double pi[6];   // u-space gradient C u + cu - A' z_rows at the solution
  double u[6];
};


// ------------------------------------------------------------------ stateless pieces of the solver
// What ipm_attempt's helpers compute from their arguments alone stands here as free functions; ipm_attempt keeps a
// one-line lambda of the old name for each (the forward keeps every kernel's device code what it was).  The helpers
// that are not here -- the row loops one slot ahead, compute_u, the AUX accessors, W^-1 and Gs -- and the phases of the
// iteration stay in ipm_attempt's body: moved out, each changed some kernel's code (profiles/ipm_phases.md).
//
// G y and G' z of a cone block (layout above)
DAT_HD void cone_G(double sec, const double* yy, double* o) {
  o[0] = -yy[2]; o[1] = -sec * yy[2]; o[2] = -yy[0]; o[3] = -yy[1]; o[4] = -yy[2];
  o[5] = 0.0; o[6] = -yy[0]; o[7] = -yy[1]; o[8] = -yy[2];
}
DAT_HD void cone_GT(double sec, const double* z, double* o) {
  o[0] = -(z[2] + z[6]);
  o[1] = -(z[3] + z[7]);
  o[2] = -(z[0] + sec * z[1] + z[4] + z[8]);
}
// (dvl, dwl) = lin(u) without the affine offsets, and its adjoint (im = 1 / mT)
// lin / adj read Bv and JTi together, before the first product: one wait for the two records
template <class SH>
DAT_HD void ipm_lin(const SH& sh, double im, const double* u, double* dv, double* dw) {
  const auto& S = sh.get();
  double Bv[10], JTi[10];
  ldn<10>(&S.Bv[0], Bv);
  ldn<10>(&S.JTi[0], JTi);
  double t[3];
  mv3(Bv, u + 3, t);
  dv[0] = im * u[0] + t[0]; dv[1] = im * u[1] + t[1]; dv[2] = im * u[2] + t[2];
  mv3(JTi, u + 3, dw);
}
template <class SH>
DAT_HD void ipm_adj(const SH& sh, double im, const double* gv, const double* gw, double* o) {
  const auto& S = sh.get();
  double Bv[10], JTi[10];
  ldn<10>(&S.Bv[0], Bv);
  ldn<10>(&S.JTi[0], JTi);
  double t[3], s[3];
  mtv3(Bv, gv, t);
  mtv3(JTi, gw, s);
  o[0] = im * gv[0]; o[1] = im * gv[1]; o[2] = im * gv[2];
  o[3] = t[0] + s[0]; o[4] = t[1] + s[1]; o[5] = t[2] + s[2];
}
// K_{-i} v = K v - U_i (U_i' v), from records already in registers (K: 22 doubles, Rt0: the U-map of block 0):
// a phase reads K and the U-map once, together with what else it needs, and applies them from there
DAT_HD void ipm_KmulR(const double* K, const double* Rt0, const double* v, double* o) {
  spmv6(K, v, o);
  double t[3], t6[6];
  Ut_apply(Rt0, v, t);
  U_apply(Rt0, t, t6);
#pragma unroll
  for (int r = 0; r < 6; ++r) o[r] -= t6[r];
}
// ... reading both records first: their reads are in flight together, one wait for the product
template <class SH, class RT>
DAT_HD void ipm_Kmul(const SH& sh, const RT& rt, const double* v, double* o) {
  double K[22], Rt0[9];
  ldn<22>(&sh.get().K[0], K);
  ldn<9>(rt.get(0), Rt0);
  ipm_KmulR(K, Rt0, v, o);
}
// Row access of the solver: the row slots' coefficients and constants, read from the base rows of the
// scenario record (sh) and the agent's env rows (er) at each use.  The base-row / env-row read is written out in
// ra3, rowld and rowval on purpose: rowval calling rowld changed k_cadmm<false> and k_cadmm_tail.
template <class SH, class ER>
struct IpmRows {
  const SH& sh;
  const ER& er;
  // row coefficients a_l (base rows: two pair reads of the (a, b) record)
  DAT_HD void ra3(int l, double* a) const {
    if (l < NBASE) {
      double r4[4];
      ldn<4>(sh.get().rows[l < NBASE ? l : 0], r4);
      a[0] = r4[0]; a[1] = r4[1]; a[2] = r4[2];
    } else {
      er.a3(l >= NBASE ? l - NBASE : 0, a);
    }
  }
  // row value a_l . (dvl or dwl) of the linear map of u
  DAT_HD double rowdot(int l, const double* dv, const double* dw) const {
    const double* x = l < NWROW ? dw : dv;
    double a[3];
    ra3(l, a);
    return a[0] * x[0] + a[1] * x[1] + a[2] * x[2];
  }
  // coefficients and constant of row l in one visit (base rows: two pair reads of the (a, b) record;
  // env rows: two pair fields)
  DAT_HD void rowld(int l, double* a, double& b) const {
    if (l < NBASE) {
      double r4[4];
      ldn<4>(sh.get().rows[l < NBASE ? l : 0], r4);
      a[0] = r4[0]; a[1] = r4[1]; a[2] = r4[2];
      b = r4[3];
    } else {
      er.ab(l >= NBASE ? l - NBASE : 0, a, b);
    }
  }
  static DAT_HD double dot3x(int l, const double* a, const double* v, const double* w) {
    const double* x = l < NWROW ? w : v;
    return a[0] * x[0] + a[1] * x[1] + a[2] * x[2];
  }
  // a_l . (dvl or dwl) + b_l
  DAT_HD double rowval(int l, const double* dv, const double* dw) const {
    const double* x = l < NWROW ? dw : dv;
    double a[3], b;
    if (l < NBASE) {
      double r4[4];
      ldn<4>(sh.get().rows[l < NBASE ? l : 0], r4);
      a[0] = r4[0]; a[1] = r4[1]; a[2] = r4[2];
      b = r4[3];
    } else {
      er.ab(l >= NBASE ? l - NBASE : 0, a, b);
    }
    return (a[0] * x[0] + a[1] * x[1] + a[2] * x[2]) + b;
  }
  // ... of a row record already in registers
  static DAT_HD double rowval_r(int l, const double* a, double b, const double* dv, const double* dw) {
    const double* x = l < NWROW ? dw : dv;
    return (a[0] * x[0] + a[1] * x[1] + a[2] * x[2]) + b;
  }
};

// Solve the reduced QP. MODE_CADMM: NB = 1, implicit free blocks through (K, atil, rho);
// MODE_DD: NB = 1, w = (F_i, M_i) free with linear cost cw; MODE_CENT: NB = n, no w.
// NR: row slots processed (NBASE .. DAT_MAXROW); every active env row must sit in a slot < NR.
// sh / er / rt: accessors of the scenario data, the env rows and the U-maps; y0: interior initial
// guess (NB x 3, f_eq); best: lane-private record of best_size(NB) doubles.  y (NB x 3) and w (6)
// are outputs.
//
// Register economy (DESIGN.md "Register and LDS budget"): only the iterates (y, w, s, z), the
// per-iteration factors (NT scalings, D^-1, M, LU) and the current Newton direction live in
// registers.  The row loops are branch-free over all NR slots (an inactive slot is the padding
// row 0 . x + 1 >= 0 with z = 0, whose complementarity target is zeroed, so it never moves and
// adds exactly nothing); row reciprocals, primal residuals and the corrector's second-order row
// terms are recomputed where consumed instead of being kept live.
// ROB: the robust instantiation (stiff rows in augmented form, below).
template <int MODE, int NB, int NR, class SH, class ER, class RT, class RW, unsigned AUXM, class GRP, bool ROB,
          bool WS = false>
DAT_HD __attribute__((always_inline)) IPMOut ipm_attempt(const SH& sh, const ER& er, const RT& rt, const QPLane<NB>& P,
                                                          const double* y0,
                          double y[NB][3], double w[6], double* best, int max_iter, double tol, RW rw, GRP grp,
                          int start, double* wrec = nullptr, bool wson = false, int clone = 0, int nclone = 1) {
  static_assert(NR >= NBASE && NR <= DAT_MAXROW, "row slots");
  // aux slot offsets (only the AUXM groups are allocated)
  constexpr int O_SC = 0;
  constexpr int O_RK = O_SC + ((AUXM & AUX_SCAL) ? 4 : 0);
  constexpr int O_RF = O_RK + 3 * NB;
  constexpr int O_LAM = O_RK + ((AUXM & AUX_RES) ? 3 * NB + 6 : 0);
  constexpr int O_DI = O_LAM + ((AUXM & AUX_LAM) ? 9 * NB : 0);
  constexpr int O_ID0 = O_DI + 6 * NB;
  constexpr int NX = ipm_aux_doubles(NB, AUXM);
  IPMOut out;
  out.status = ST_FAILED;
  out.iters = 0;
  out.inband = 0;
  out.why = 0;
  out.refs = 0;
  out.corrs = 0;
  out.stiff = 0;
  out.merit = 1e300;
#pragma unroll
  for (int r = 0; r < 6; ++r) { out.pi[r] = 0.0; out.u[r] = 0.0; }
  if (sh.get().infeasible || P.infeasible) {
    out.status = ST_INFEASIBLE;
    return out;
  }
  const unsigned emask = P.emask << NBASE;
  if (emask >> NR) return out;  // an active row outside the instantiated slots: caller error
  const unsigned mask = (unsigned)sh.get().bmask | emask;
  const int var = P.var;
  const double sec = P.sec, kap = P.kappa;
  const double irho = 1.0 / P.rho;
  const double im = sh.get().inv_mT;
  auto act = [&](int l) -> double { return ((mask >> l) & 1u) ? 1.0 : 0.0; };
  auto Cp = [&]() { return &sh.get().C[var][0]; };
  auto cup = [&]() { return &sh.get().cu[var][0]; };
  auto rb = [&](int l) -> double { return l < NBASE ? sh.get().rows[l < NBASE ? l : 0][3] : er.b(l >= NBASE ? l - NBASE : 0); };
  // forwards to the stateless pieces above (row access, lin / adj; K_{-i} and G below)
  const IpmRows<SH, ER> rows{sh, er};
  auto dot3x = [&](int l, const double* a, const double* v, const double* w) -> double { return rows.dot3x(l, a, v, w); };
  auto rowval = [&](int l, const double* dv, const double* dw) -> double { return rows.rowval(l, dv, dw); };
  auto rowval_r = [&](int l, const double* a, double b, const double* dv, const double* dw) -> double { return rows.rowval_r(l, a, b, dv, dw); };
  auto rowld = [&](int l, double* a, double& b) { rows.rowld(l, a, b); };
  auto lin = [&](const double* u, double* dv, double* dw) { ipm_lin(sh, im, u, dv, dw); };
  auto adj = [&](const double* gv, const double* gw, double* o) { ipm_adj(sh, im, gv, gw, o); };
  // Row loops, one slot ahead ("How the IPM reads LDS"): slot l + 1's records are read before slot l is computed,
  // so a row's LDS round trip overlaps the previous row's arithmetic.  The look-ahead ends at NR - 1 at compile
  // time (nothing is read past the last slot), and a body that writes slot l's state (set_sz, ZW) does so after
  // slot l + 1 -- another slot -- was read: no read is moved across a write to its own slot.
  struct RowAB { double a[3], b; };          // coefficients and constant of a row
  struct RowRec { double s, z, a[3], b; };   // ... with its (s, z) pair
  auto for_rows_ab = [&](auto f) {
    RowAB nx;
    rowld(0, nx.a, nx.b);
#pragma unroll
    for (int l = 0; l < NR; ++l) {
      const RowAB cu = nx;
      if (l + 1 < NR) rowld(l + 1 < NR ? l + 1 : 0, nx.a, nx.b);
      f(l, cu);
    }
  };
  auto rows_adj = [&](auto zz, double* o) {  // o = A' zz (u-space); zz(l): row multiplier
    double gv[3] = {0, 0, 0}, gw[3] = {0, 0, 0};
    for_rows_ab([&](int l, const RowAB& r) {
      double* g = l < NWROW ? gw : gv;
      const double zv = zz(l);
      const double* a = r.a;
      g[0] += zv * a[0]; g[1] += zv * a[1]; g[2] += zv * a[2];
    });
    adj(gv, gw, o);
  };
  auto KmulR = [&](const double* K, const double* Rt0, const double* v, double* o) { ipm_KmulR(K, Rt0, v, o); };
  auto Kmul = [&](const double* v, double* o) { ipm_Kmul(sh, rt, v, o); };
  auto Gy = [&](const double* yy, double* o) { cone_G(sec, yy, o); };
  auto GTz = [&](const double* z, double* o) { cone_GT(sec, z, o); };
  const double mfz = P.min_fz, mxf = P.max_f;
  // primal residual of cone block k at the current iterate: G y + s - h
  double sk[NB][9], zk[NB][9];
  typename RW::template Store<NR, NX> rst(rw);  // row slacks / duals / Newton row terms (registers or LDS)
  auto SL = [&](int l) -> decltype(auto) { return rst.s(l); };
  auto ZL = [&](int l) -> decltype(auto) { return rst.z(l); };
  // the row loop one slot ahead (for_rows_ab), with the row's (s, z) pair
  auto for_rows = [&](auto f) {
    RowRec nx;
    rst.sz(0, nx.s, nx.z);
    rowld(0, nx.a, nx.b);
#pragma unroll
    for (int l = 0; l < NR; ++l) {
      const RowRec cu = nx;
      if (l + 1 < NR) {
        rst.sz(l + 1 < NR ? l + 1 : 0, nx.s, nx.z);
        rowld(l + 1 < NR ? l + 1 : 0, nx.a, nx.b);
      }
      f(l, cu);
    }
  };
  // per-iteration quantities: registers, or the store's aux slots (AUXM)
  double nh_r = 0.0, nq_r = 0.0, bm_r = 0.0, bk_r = 0.0;
  double rk_r[(AUXM & AUX_RES) ? 1 : 3 * NB], rf_r[(AUXM & AUX_RES) ? 1 : 6];
  double lam_r[(AUXM & AUX_LAM) ? 1 : 9 * NB];
  double di_r[(AUXM & AUX_DINV) ? 1 : 6 * NB], id0_r[(AUXM & AUX_DINV) ? 1 : NB];
  auto NH = [&]() -> decltype(auto) {
    if constexpr ((AUXM & AUX_SCAL) != 0) return rst.x(O_SC + 0); else return (nh_r);
  };
  auto NQ = [&]() -> decltype(auto) {
    if constexpr ((AUXM & AUX_SCAL) != 0) return rst.x(O_SC + 1); else return (nq_r);
  };
  auto BM = [&]() -> decltype(auto) {  // best merit seen (divergence stop)
    if constexpr ((AUXM & AUX_SCAL) != 0) return rst.x(O_SC + 2); else return (bm_r);
  };
  auto BK = [&]() -> decltype(auto) {  // merit of the recorded in-band iterate
    if constexpr ((AUXM & AUX_SCAL) != 0) return rst.x(O_SC + 3); else return (bk_r);
  };
  auto RK = [&](int k, int c) -> decltype(auto) {
    if constexpr ((AUXM & AUX_RES) != 0) return rst.x(O_RK + 3 * k + c); else return (rk_r[3 * k + c]);
  };
  auto RF = [&](int r) -> decltype(auto) {
    if constexpr ((AUXM & AUX_RES) != 0) return rst.x(O_RF + r); else return (rf_r[r]);
  };
  auto LAM = [&](int k, int j) -> decltype(auto) {
    if constexpr ((AUXM & AUX_LAM) != 0) return rst.x(O_LAM + 9 * k + j); else return (lam_r[9 * k + j]);
  };
  auto DI = [&](int k, int j) -> decltype(auto) {
    if constexpr ((AUXM & AUX_DINV) != 0) return rst.x(O_DI + 6 * k + j); else return (di_r[6 * k + j]);
  };
  auto ID0 = [&](int k) -> decltype(auto) {
    if constexpr ((AUXM & AUX_DINV) != 0) return rst.x(O_ID0 + k); else return (id0_r[k]);
  };
  auto lam4 = [&](int k, int j0, double* o) {  // lambda_k[j0 .. j0 + 3]
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = LAM(k, j0 + j);
  };
  auto dinv = [&](int k, double* o) {
#pragma unroll
    for (int j = 0; j < 6; ++j) o[j] = DI(k, j);
  };
  auto rzk_of = [&](int k, double* o) {
    Gy(y[k], o);
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] += sk[k][j];
    o[0] += mfz;
    o[5] -= mxf;
  };
  auto compute_u = [&](double* uo) {
#pragma unroll
    for (int r = 0; r < 6; ++r) uo[r] = (MODE == MODE_CENT) ? 0.0 : w[r];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      double t[6];
      U_apply(rt.get(k), y[k], t);
#pragma unroll
      for (int r = 0; r < 6; ++r) uo[r] += t[r];
    }
    if constexpr (GRP::on) {
#pragma unroll
      for (int r = 0; r < 6; ++r) uo[r] = grp.sum(uo[r]);  // (MODE_CENT: no w)
    }
  };

  // ---------------- initial point
  // The tuned start and step fraction for the C-ADMM agent QPs of a step's first ADMM pass and of
  // scenarios whose previous step took <= 3 passes (P.tuned: the warm closed loop, whose multipliers
  // are O(1e-2)); the conservative ones for the later passes of long ADMM runs (C2 / C5, cold random
  // inputs and 17-28 passes: the tuned start everywhere took C2 13 -> 20 ms and C5 81 -> 118 ms per
  // step), DD agent QPs (C3 29 -> 39 ms) and the centralized QP (also the rigid payload on the same
  // kernel, whose Jl^-1 ~ 50 grades the Newton systems)
  // start 0: conservative (as above), 1: tuned (C-ADMM), 2: the conservative start scaled by 10 (the
  // second start of a DD / centralized solve that ended outside Clarabel's tolerance, see ipm_solve)
  const bool TUNED = MODE == MODE_CADMM && start == 1;
  const double SCL = start == 2 ? 10.0 : 1.0;
  const double S0 = SCL * (TUNED ? IPM_S0 : MODE == MODE_DD ? DD_S0 : 1.0);
  const double Z0 = SCL * (TUNED ? IPM_Z0 : MODE == MODE_DD ? DD_Z0 : 1.0);
  const double ETA = TUNED ? IPM_ETA : MODE == MODE_DD ? DD_ETA : 0.99;
#pragma unroll
  for (int k = 0; k < NB; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) y[k][c] = y0[3 * k + c];
    double g[9];
    Gy(y[k], g);
#pragma unroll
    for (int j = 0; j < 9; ++j) sk[k][j] = -g[j];
    sk[k][0] -= mfz;
    sk[k][5] += mxf;
    // shift into the interior if the guess is not strictly feasible
    double m1 = sk[k][0], m2 = sk[k][1] - sqrt(sk[k][2] * sk[k][2] + sk[k][3] * sk[k][3] + sk[k][4] * sk[k][4]);
    double m3 = sk[k][5] - sqrt(sk[k][6] * sk[k][6] + sk[k][7] * sk[k][7] + sk[k][8] * sk[k][8]);
    double mn = fmin(m1, fmin(m2, m3));
    if (mn < 1e-3) { sk[k][0] += S0 - mn; sk[k][1] += S0 - mn; sk[k][5] += S0 - mn; }
#pragma unroll
    for (int j = 0; j < 9; ++j) zk[k][j] = 0.0;
    zk[k][0] = Z0; zk[k][1] = Z0; zk[k][5] = Z0;
  }
#pragma unroll
  for (int l = 0; l < NR; ++l) ZL(l) = Z0 * act(l);  // (the slack half of the pair is written below)
#pragma unroll
  for (int r = 0; r < 6; ++r) w[r] = 0.0;
  // C-ADMM: the free aggregate starts at its unconstrained minimiser without the u-coupling,
  // w = atil (the infeasible start lets the Newton steps restore rho (w - atil) + K_{-i} pi = 0).
  // A consistent start through a 6x6 LU of (rho I + K C) took the same iteration count and held
  // ~1 KB/lane more spill frame (C4 A/B: k_cadmm 8.9 -> 7.7 ms without it).
  if (MODE == MODE_CADMM) {
#pragma unroll
    for (int r = 0; r < 6; ++r) w[r] = P.atil[r];
  }
  {
    double u[6], dv[3], dw[3];
    compute_u(u);
    lin(u, dv, dw);
#pragma unroll
    for (int l = 0; l < NR; ++l) SL(l) = fmax(rowval(l, dv, dw), S0);
  }
  if constexpr (WS) {
    static_assert(NB == 1 && NR <= DAT_MAXROW, "warm start: C-ADMM agent QP");
    if (start == 3) {
      // (s, z) -> (s + d, z + d) with (s + d)(z + d) >= mu (WS_MU; DD_WS_MU for the DD agent QPs)
      constexpr double mu = MODE == MODE_DD ? DD_WS_MU : WS_MU;
      auto push = [](double s, double z) -> double {
        const double p = s * z;
        if (!(p < mu)) return 0.0;
        const double t = s + z;
        return 0.5 * (sqrt(t * t + 4.0 * (mu - p)) - t);
      };
#pragma unroll
      for (int c = 0; c < 3; ++c) y[0][c] = wrec[1 + c];
#pragma unroll
      for (int r = 0; r < 6; ++r) w[r] = wrec[4 + r];
      double g[9];
      Gy(y[0], g);
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        sk[0][j] = -g[j];
        zk[0][j] = wrec[19 + j];
      }
      sk[0][0] -= mfz;
      sk[0][5] += mxf;
      {
        const double d = push(fmax(sk[0][0], 0.0), fmax(zk[0][0], 0.0));
        sk[0][0] = fmax(sk[0][0], 0.0) + d;
        zk[0][0] = fmax(zk[0][0], 0.0) + d;
      }
#pragma unroll
      for (int b = 1; b <= 5; b += 4) {
        const double ms = sk[0][b] - sqrt(sk[0][b + 1] * sk[0][b + 1] + sk[0][b + 2] * sk[0][b + 2] + sk[0][b + 3] * sk[0][b + 3]);
        const double mz = zk[0][b] - sqrt(zk[0][b + 1] * zk[0][b + 1] + zk[0][b + 2] * zk[0][b + 2] + zk[0][b + 3] * zk[0][b + 3]);
        const double d = push(fmax(ms, 0.0), fmax(mz, 0.0));
        sk[0][b] += d - fmin(ms, 0.0);
        zk[0][b] += d - fmin(mz, 0.0);
      }
      double u[6], dv[3], dw[3];
      compute_u(u);
      lin(u, dv, dw);
#pragma unroll
      for (int l = 0; l < NR; ++l) {
        const double sl = fmax(rowval(l, dv, dw), 0.0), zl = fmax(wrec[28 + DAT_MAXROW + l], 0.0);
        const double d = act(l) * push(sl, zl);
        rst.set_sz(l, act(l) > 0.0 ? sl + d : fmax(rowval(l, dv, dw), S0), act(l) * (zl + d));
      }
    }
  }

  // scales for the relative stopping rule
  {
    double nh = 1.0 + fmax(mfz, mxf), nq = 1.0;
#pragma unroll
    for (int l = 0; l < NR; ++l) nh = fmax(nh, 1.0 + act(l) * fabs(rb(l)));
    {
      double nb = 1.0;
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) nb = fmax(nb, 1.0 + fabs(P.q[k][c]));
      nq = fmax(nq, grp.max(nb));
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) nq = fmax(nq, 1.0 + fabs(cup()[r]));
    NH() = nh;
    NQ() = nq;
  }

  // best in-band iterate (merit of the recorded one) and the best merit seen (divergence stop)
  BM() = 1e300;
  BK() = 1e300;
  out.status = ST_INACCURATE;  // until converged (or failed on non-finite data)
  const double ideg = 1.0 / (double)(3 * grp.nblk(NB) + __builtin_popcount(mask));
  int bk_it = 0;  // WS: the iteration of the last halving of the best in-band merit (stall exit)
  // WS: the current iterate into the warm-start record (the next ADMM pass's start)
  auto record = [&]() {
    if constexpr (WS) {
      if (wrec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) wrec[1 + c] = y[0][c];
#pragma unroll
        for (int r = 0; r < 6; ++r) wrec[4 + r] = w[r];
#pragma unroll
        for (int j = 0; j < 9; ++j) { wrec[10 + j] = sk[0][j]; wrec[19 + j] = zk[0][j]; }
#pragma unroll
        for (int l = 0; l < NR; ++l) {
          double sl, zl;
          rst.sz(l, sl, zl);
          wrec[28 + l] = sl;
          wrec[28 + DAT_MAXROW + l] = zl;
        }
        wrec[0] = 1.0;
      }
    }
  };

  DAT_PHASE_INIT(0);
  for (int it = 0;; ++it) {
    DAT_PHASE(1);
    // ------------- residuals
    double dv[3], dw[3];
    double dres = 0.0, pres = 0.0, gap = 0.0;
    double chk = 0.0;  // plain sum of every residual entry: NaN / Inf propagate (fmax drops NaN)
    // primal objective of the iterate (constants dropped, as cvxpy hands it to the solver): the scale
    // of the relative gap test
    double pobj = 0.0;
    {
      double u[6], pi[6], az[6];
      compute_u(u);
      lin(u, dv, dw);
      spmv6(Cp(), u, pi);
      rows_adj(ZL, az);
      {
        double cu6[6];
        ldn<6>(cup(), cu6);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          pobj += u[r] * (0.5 * pi[r] + cu6[r]);
          pi[r] += cu6[r] - az[r];
        }
      }
      // the cone blocks' parts (reduced over a lane group, GRP) before the replicated ones
      double pobj_b = 0.0;
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        double ut[3], gz[3];
        Ut_apply(rt.get(k), pi, ut);
        GTz(zk[k], gz);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double r = kap * y[k][c] + P.q[k][c] + ut[c] + gz[c];
          pobj_b += y[k][c] * (0.5 * kap * y[k][c] + P.q[k][c]);
          RK(k, c) = r;
          dres = fmax(dres, fabs(r));
          chk += r;
        }
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        double rz[9];
        rzk_of(k, rz);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          pres = fmax(pres, fabs(rz[j]));
          chk += rz[j];
          gap += sk[k][j] * zk[k][j];
        }
      }
      if constexpr (GRP::on) {
        dres = grp.max(dres);
        pres = grp.max(pres);
        chk = grp.sum(chk);
        gap = grp.sum(gap);
        pobj_b = grp.sum(pobj_b);
      }
      pobj += pobj_b;
      {
        double Rf[6];
        if (MODE == MODE_CADMM) {
          // free blocks f_j = a_j - U_j' pi / rho: sum_j rho/2 ||f_j||^2 - rho a_j . f_j
          //   = pi' K_{-i} pi / (2 rho) - rho/2 sum_j ||a_j||^2
          double kp[6];
          Kmul(pi, kp);
          double pkp = 0.0;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            Rf[r] = P.rho * (w[r] - P.atil[r]) + kp[r];
            pkp += pi[r] * kp[r];
          }
          pobj += 0.5 * (pkp * irho - P.rho * P.a2);
        } else if (MODE == MODE_DD) {
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            Rf[r] = pi[r] + P.cw[r];
            pobj += P.cw[r] * w[r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 6; ++r) Rf[r] = 0.0;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          RF(r) = Rf[r];
          dres = fmax(dres, fabs(Rf[r]));
          chk += Rf[r];
        }
      }
      for_rows([&](int l, const RowRec& r) {
        const double sl = r.s, zl = r.z;
        const double rl = sl - (rowval_r(l, r.a, r.b, dv, dw));
        pres = fmax(pres, fabs(rl));
        chk += rl;
        gap += sl * zl;
      });
      out.iters = it;
      if (!(fabs(chk + gap) < 1e300)) {  // NaN or Inf anywhere in the residuals
        // at the initial point: the problem data itself is not finite (the solver-exception
        // branch); later: a numerical breakdown of a finite problem (not solved)
        out.status = it == 0 ? ST_FAILED : ST_INACCURATE;
        out.why = 1;
        break;
      }
      const double nh = NH(), nq = NQ();
      // complementarity gap, absolute or relative to the objective as Clarabel tests it (gap_abs or
      // gap_rel): converged when gap < 10 tol or gap < tol / 10 |pobj| (at the default tol = 1e-10: 1e-9
      // absolute, or the oracle's own 1e-11 relative rule), i.e. the scaled gap gap / max(1, |pobj| / 100)
      // below 10 tol.  With multipliers ~1e3-1e4 (a stalled ADMM loop, |pobj| ~1e4-1e5) an absolute gap
      // of 1e-9 lies below what the Newton systems resolve; well-scaled QPs (|pobj| <= 100) keep the
      // absolute rule.
      const double grel = gap * frcp(fmax(1.0, 0.01 * fabs(pobj)));
      double merit = fmax(fmax(pres / nh, dres / nq), grel);
#ifdef DAT_IPM_TRACE
      printf("ipm it %2d pres %.3e dres %.3e gap %.3e merit %.3e pobj %.3e\n", it, pres / nh, dres / nq, grel, merit,
             pobj);
#endif
      if (pres < tol * nh && dres < tol * nq && grel < 10.0 * tol) {
        out.status = ST_OPTIMAL;
        out.merit = merit;
#pragma unroll
        for (int r = 0; r < 6; ++r) { out.pi[r] = pi[r]; out.u[r] = u[r]; }
        record();  // the converged iterate: the next pass's warm start
        DAT_PHASE(8);
        return out;
      }
      // Only an in-band iterate (scaled residuals < 1e-7, relative gap < 1e-6) can be returned: a solve
      // that ends out of band is INACCURATE and the callers hold their previous solution instead, so
      // out-of-band iterates are never recorded (the record is written in the last one or two
      // iterations of a stalling solve, not at every iteration).  Its merit is measured as Clarabel
      // measures convergence (residuals, and the gap absolute or relative to the objective, whichever
      // is smaller: max(1, |pobj|) scaling), so inband_loose counts exactly the accepts outside
      // Clarabel's own tolerance.
      const double mclr = fmax(fmax(pres / nh, dres / nq), gap * frcp(fmax(1.0, fabs(pobj))));
      const bool band = fmax(pres / nh, dres / nq) < 1e-7 && mclr < 1e-6;
      const bool prog = band && mclr < 0.5 * BK();  // (WS: the stall exit below)
      if (band && mclr < BK()) {
        BK() = mclr;
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
          for (int c = 0; c < 3; ++c) best[3 * k + c] = y[k][c];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          best[3 * NB + r] = w[r];
          best[3 * NB + 6 + r] = pi[r];
          best[3 * NB + 12 + r] = u[r];
        }
      }
      if (WS && wson) {
        // stall exit (the tail kernel): an in-band iterate WS_STALL_TOL (ten times inside Clarabel's tolerance)
        // is recorded and the merit has not halved in WS_STALL_ITS iterations -- the Newton systems of a stalled
        // ADMM loop's agent QP resolve no further; its best in-band iterate is returned (OPTIMAL, in band)
        if (prog) bk_it = it;
        if (BK() <= WS_STALL_TOL && it - bk_it >= WS_STALL_ITS) {
          out.why = 7;
          record();  // the current iterate (in band): the next pass's warm start
          break;
        }
      }
      BM() = fmin(BM(), merit);
      if ((it >= 4 && merit > IPM_DIVERGE * BM()) || it >= max_iter) {
        out.why = 2;
        break;
      }
      if (it >= max_iter) break;
    }

    // ------------- NT scaling of the cone blocks
    DAT_PHASE(2);
#if defined(DAT_IPM_STATS) && !defined(__HIP_DEVICE_COMPILE__)
    g_maxw = 0.0;
#endif
    SocScale S1[NB], S2[NB];
    bool okc = true;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (ROB) {
        // a second-order cone iterate that rounding put on (or past) the boundary: back inside by a few ulps of
        // its axis (the step rule keeps it strictly inside in exact arithmetic).  Without it the robust solver
        // stopped at the NT scaling (why 3) on the stall QPs the 10 s C4 loop accepted beyond Clarabel's 1e-8 (20
        // of 20 captured, tests/golden/ref_loose_caps.npz); with it all 20 converge to 1e-11.
#pragma unroll
        for (int b0 = 1; b0 <= 5; b0 += 4) {
          double* vv[2] = {sk[k] + b0, zk[k] + b0};
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            double* v = vv[q];
            const double n1 = sqrt(v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
            if (!(v[0] - n1 > 1e-14 * n1)) v[0] = n1 * (1.0 + 1e-14) + 1e-300;
          }
        }
      }
      ID0(k) = sqrt(zk[k][0] * frcp(sk[k][0]));  // 1 / d0, d0 = sqrt(s0 / z0)
      LAM(k, 0) = sqrt(sk[k][0] * zk[k][0]);
      okc = okc && soc_scaling(sk[k] + 1, zk[k] + 1, S1[k]) && soc_scaling(sk[k] + 5, zk[k] + 5, S2[k]);
      double l1[4], l2[4];
      soc_apply(S1[k], zk[k] + 1, l1, false);
      soc_apply(S2[k], zk[k] + 5, l2, false);
#pragma unroll
      for (int j = 0; j < 4; ++j) { LAM(k, 1 + j) = l1[j]; LAM(k, 5 + j) = l2[j]; }
    }
#ifdef DAT_IPM_TRACE
    for (int k = 0; k < NB; ++k)
      printf("    cone s %.2e %.2e %.2e z %.2e %.2e %.2e | eta1 %.2e eta2 %.2e | rows z/s %.2e %.2e %.2e\n", sk[k][0],
             sk[k][1] - sqrt(sk[k][2] * sk[k][2] + sk[k][3] * sk[k][3] + sk[k][4] * sk[k][4]),
             sk[k][5] - sqrt(sk[k][6] * sk[k][6] + sk[k][7] * sk[k][7] + sk[k][8] * sk[k][8]), zk[k][0],
             zk[k][1] - sqrt(zk[k][2] * zk[k][2] + zk[k][3] * zk[k][3] + zk[k][4] * zk[k][4]),
             zk[k][5] - sqrt(zk[k][6] * zk[k][6] + zk[k][7] * zk[k][7] + zk[k][8] * zk[k][8]), S1[k].eta, S2[k].eta,
             (double)ZL(0) / (double)SL(0), (double)ZL(1) / (double)SL(1), (double)ZL(2) / (double)SL(2));
#endif
    if constexpr (GRP::on) okc = grp.min(okc ? 1.0 : 0.0) > 0.5;
    if (!okc) {
      out.why = 3;
      break;
    }
    auto winv = [&](int k, const double* v, double* o) {  // W_k^-1 v
      o[0] = v[0] * ID0(k);
      soc_apply(S1[k], v + 1, o + 1, true);
      soc_apply(S2[k], v + 5, o + 5, true);
    };
    // Gs = W^-1 G applied to a 3-vector / its transpose applied to a 9-vector
    auto gs_mul = [&](int k, const double* v, double* o) {
      double g[9];
      Gy(v, g);
      winv(k, g, o);
    };
    auto gs_tmul = [&](int k, const double* t, double* o) {
      double g[9];
      winv(k, t, g);
      GTz(g, o);
    };
    // D_k = kappa I + Gs'Gs through its QR square-root factor (qr_cone: forming D cancels once an active
    // cone makes Gs stiff); DI holds the factor, applied by dsolve3
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      double gc[3][9];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double e[3] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0};
        gs_mul(k, e, gc[c]);
      }
      double Rd[6];
      okc = okc && qr_cone(kap, gc, Rd);
#pragma unroll
      for (int j = 0; j < 6; ++j) DI(k, j) = Rd[j];
    }
    if constexpr (GRP::on) okc = grp.min(okc ? 1.0 : 0.0) > 0.5;
    if (!okc) {
      out.why = 4;
      break;
    }
    DAT_PHASE(3);
    // M = Lm Lm' (Cholesky; M is SPD: C carries k_f, k_m > 0) and, for CADMM / CENT, the Cholesky
    // factor Ln of the SPD matrix N = I + Lm' T Lm, so that (I + M T)^-1 M = Lm N^-1 Lm' =: P.  N has
    // every eigenvalue >= 1 however large active rows make M, so the factorisation stays well
    // conditioned without a pivoted nonsymmetric LU; only P (21 doubles) is kept for the solves.
    // DD: Lm alone (reciprocal diagonal, for chol6_solve).
    // Stiff rows.  Near the solution an active row's barrier weight z/s grows without bound; inside a
    // stalled ADMM loop (multipliers ~1e3-1e4, rows with tiny coefficients) it reaches 1e10-1e22.  Folded
    // into M = C + A'(Z/S)A it wipes out C's digits, and the row's dual direction dz = zw - (z/s) a.du is
    // a difference of huge terms.  So the first IPM_NSTIFF rows (slot order) whose weight exceeds
    // IPM_STIFF_W stay out of M; their dual directions are unknowns of a small augmented system
    //   a_l . lin(du) + (s_l / z_l) dz_l = g_l      (row primal + complementarity, no 1/s anywhere)
    // solved by a Schur complement on the stiff rows: du = du0 + sum_l dz_l H abar_l, where du0 is the
    // core solve without them and H abar_l a core solve with the row's u-space coefficient as bu (the
    // columns, once per iteration, kept in the lane's scratch record behind `best`).  Without stiff rows
    // (every well-scaled QP) nothing changes.
    unsigned smask = 0u;  // stiff row slots (the rows' data: the scratch record behind `best`)
    double* const hcol = best + best_rec(NB);                    // [j][dy (3 NB), dw (6), du (6)]
    double* const srec = hcol + IPM_NSTIFF * stiff_col(NB);      // [j][a0 a1 a2 on_dwl e g dz tmp]
    double* const sfac = srec + IPM_NSTIFF * STIFF_ROW;          // Cholesky factor of S
    // DD: Cholesky factor of M;  CADMM / CENT: P = Lm N^-1 Lm' (schur_P).  WS (the tail kernel, one scenario
    // per workgroup, latency-bound): kept in the lane's scratch record (LDS there) across the iteration's solves
    // instead of 42 registers of a frame that spills (stall fixture, same-call A/B: 41.8 / 33.7 -> 39.1 / 30.6 ms per
    // stalled step; the cones' s, z and the Newton step's cone terms there as well measured no better, or worse)
    double LmR[21];
    double* const Lm = WS && MODE == MODE_CADMM ? best + best_size(NB) - FM_DOUBLES : LmR;  // (DD: HBM records)
    {
      double Mm[21];
      // M = C + sum_l (z/s) a_l a_l' (u-space, packed), assembled in (dvl, dwl) coordinates
      {
        double Xv[6] = {0, 0, 0, 0, 0, 0}, Xw[6] = {0, 0, 0, 0, 0, 0};
        for_rows([&](int l, const RowRec& rr) {
          const double sl = rr.s, zl = rr.z;
          double wgt = zl * frcp(sl);
          DAT_STAT_W(act(l) * wgt);
          const double* a3v = rr.a;
          if (ROB && act(l) > 0.0 && wgt > IPM_STIFF_W && __builtin_popcount(smask) < IPM_NSTIFF) {
            double* r = srec + __builtin_popcount(smask) * STIFF_ROW;
            r[0] = a3v[0]; r[1] = a3v[1]; r[2] = a3v[2];
            r[3] = l < NWROW ? 1.0 : 0.0;
            r[4] = sl * frcp(zl);
            smask |= 1u << l;
            wgt = 0.0;
          }
          double* X = l < NWROW ? Xw : Xv;
          const double a0 = a3v[0], a1 = a3v[1], a2 = a3v[2];
          X[0] += wgt * a0 * a0; X[1] += wgt * a0 * a1; X[2] += wgt * a0 * a2;
          X[3] += wgt * a1 * a1; X[4] += wgt * a1 * a2; X[5] += wgt * a2 * a2;
        });
        // Av = [im I, Bv];  Av' Xv Av = [[im^2 Xv, im Xv Bv], [., Bv' Xv Bv]];  Aw = [0, JTi]
        // (Bv, JTi and C are read together: one wait for the three records)
        const auto& S = sh.get();
        double XB[9], XJ[9], Bv[10], JTi[10], C[22];
        ldn<10>(S.Bv, Bv);
        ldn<10>(S.JTi, JTi);
        ldn<22>(&S.C[var][0], C);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            XB[3 * r + c] = Xv[sp3(r, 0)] * Bv[c] + Xv[sp3(r, 1)] * Bv[3 + c] + Xv[sp3(r, 2)] * Bv[6 + c];
            XJ[3 * r + c] = Xw[sp3(r, 0)] * JTi[c] + Xw[sp3(r, 1)] * JTi[3 + c] + Xw[sp3(r, 2)] * JTi[6 + c];
          }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (c >= r) {
              Mm[sp6(r, c)] = C[sp6(r, c)] + im * im * Xv[sp3(r, c)];
              double s = C[sp6(3 + r, 3 + c)];
#pragma unroll
              for (int k2 = 0; k2 < 3; ++k2) s += Bv[3 * k2 + r] * XB[3 * k2 + c] + JTi[3 * k2 + r] * XJ[3 * k2 + c];
              Mm[sp6(3 + r, 3 + c)] = s;
            }
            Mm[sp6(r, 3 + c)] = C[sp6(r, 3 + c)] + im * XB[3 * r + c];
          }
      }
      if (MODE == MODE_DD) {
        if (!chol6(Mm, Lm)) {
          out.why = 5;
          break;
        }
      } else {
        if (!chol6_lower(Mm, Lm)) {
          out.why = 5;
          break;
        }
        // T = sum_k U_k D_k^-1 U_k' (+ K_{-i} / rho)
        double T[21];
        if (MODE == MODE_CADMM) {
          double K[22], Rd[6], Dm[6], Rt0[9];  // (K, the cone factor and the U-map: read together)
          ldn<22>(&sh.get().K[0], K);
          dinv(0, Rd);
          ldn<9>(rt.get(0), Rt0);
#pragma unroll
          for (int k = 0; k < 21; ++k) T[k] = K[k] * irho;
          // K_{-i}/rho + U_i Dinv U_i' = K/rho + U_i (Dinv - I/rho) U_i'
          dinv_explicit(Rd, Dm);
          Dm[0] -= irho;
          Dm[3] -= irho;
          Dm[5] -= irho;
          add_UDUt(T, Rt0, Dm, 1.0);
        } else {
#pragma unroll
          for (int k = 0; k < 21; ++k) T[k] = 0.0;
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            double Rd[6], Di[6];
            dinv(k, Rd);
            dinv_explicit(Rd, Di);
            add_UDUt(T, rt.get(k), Di, 1.0);
          }
          if constexpr (GRP::on) {
#pragma unroll
            for (int k = 0; k < 21; ++k) T[k] = grp.sum(T[k]);
          }
        }
        double Nn[21], Ln[21];
        ltl_plus_identity(Lm, T, Nn);
        if (!chol6(Nn, Ln)) {
          out.why = 6;
          break;
        }
        double Pm[21];
        schur_P(Lm, Ln, Pm);
#pragma unroll
        for (int k = 0; k < 21; ++k) Lm[k] = Pm[k];
      }
    }

    // core structured solve of (D + U'MU) dx = b (CADMM/CENT) or its DD analogue.  bu: u-space
    // part of the right-hand side (has_bu = false: zero); acc: add the solution to the outputs.
    auto core = [&](const double bk[NB][3], const double* Rfr, const double* bu, bool has_bu, bool acc,
                    double dyo[NB][3], double* dwo, double* duo) {
      double dyn[NB][3], dwn[6], dun[6];
      // the blocks' U-maps and cone factors, and (C-ADMM) the aggregate K: read once, first, so that the reads
      // are in flight together; the products below take the records from registers ("How the IPM reads LDS")
      double Rtk[NB][9], Rdk[NB][6], Kc[22];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        ldn<9>(rt.get(k), Rtk[k]);
        dinv(k, Rdk[k]);
      }
      if (MODE == MODE_CADMM) ldn<22>(&sh.get().K[0], Kc);
      if (MODE == MODE_DD) {
#pragma unroll
        for (int r = 0; r < 6; ++r) dun[r] = -Rfr[r] + (has_bu ? bu[r] : 0.0);
        chol6_solve(Lm, dun);
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          double t[3], v[3];
          Ut_apply(Rtk[k], Rfr, t);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c] = bk[k][c] + t[c];
          dsolve3(Rdk[k], v, dyn[k]);
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) dwn[r] = dun[r];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          double t[6];
          U_apply(Rtk[k], dyn[k], t);
#pragma unroll
          for (int r = 0; r < 6; ++r) dwn[r] -= t[r];
        }
      } else {
        double bk2[NB][3], yv[6] = {0, 0, 0, 0, 0, 0}, g6[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          double t[3] = {0, 0, 0}, v[3], ut[6];
          if (has_bu) Ut_apply(Rtk[k], bu, t);
#pragma unroll
          for (int c = 0; c < 3; ++c) bk2[k][c] = bk[k][c] + t[c];
          dsolve3(Rdk[k], bk2[k], v);
          U_apply(Rtk[k], v, ut);
#pragma unroll
          for (int r = 0; r < 6; ++r) yv[r] += ut[r];
        }
        if constexpr (GRP::on) {
#pragma unroll
          for (int r = 0; r < 6; ++r) yv[r] = grp.sum(yv[r]);
        }
        if (MODE == MODE_CADMM) {
          if (has_bu) KmulR(Kc, Rtk[0], bu, g6);
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            g6[r] -= Rfr[r];  // g6 = -Rf + K_{-i} bu
            yv[r] += g6[r] * irho;
          }
        }
        // tau = (I + M T)^-1 M yv = Lm N^-1 Lm' yv = P yv
        double tau[6];
        spmv6(Lm, yv, tau);
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          double t[3], v[3];
          Ut_apply(Rtk[k], tau, t);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c] = bk2[k][c] - t[c];
          dsolve3(Rdk[k], v, dyn[k]);
        }
        if (MODE == MODE_CADMM) {
          double kt[6];
          KmulR(Kc, Rtk[0], tau, kt);
#pragma unroll
          for (int r = 0; r < 6; ++r) dwn[r] = (g6[r] - kt[r]) * irho;
        } else {
#pragma unroll
          for (int r = 0; r < 6; ++r) dwn[r] = 0.0;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) dun[r] = (MODE == MODE_CADMM) ? dwn[r] : 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          double t[6];
          U_apply(Rtk[k], dyn[k], t);
#pragma unroll
          for (int r = 0; r < 6; ++r) dun[r] += t[r];
        }
        if constexpr (GRP::on) {  // (MODE_CENT: no w)
#pragma unroll
          for (int r = 0; r < 6; ++r) dun[r] = grp.sum(dun[r]);
        }
      }
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) dyo[k][c] = (acc ? dyo[k][c] : 0.0) + dyn[k][c];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        dwo[r] = (acc ? dwo[r] : 0.0) + dwn[r];
        duo[r] = (acc ? duo[r] : 0.0) + dun[r];
      }
    };

    // Newton direction for complementarity targets rsk (cones, scaled) and, for the rows,
    // rc_l = s_l z_l + cadd_l (cadd = 0 for the predictor; the corrector's second-order term is
    // formed in place from the predictor's row direction ddva/ddwa and its zw).  Outputs: dy, dw,
    // du, scaled dz of the cones (dzs_k), lam \ rsk (lrs_k, so dss_k = -lrs_k - dzs_k) and zw
    // (row dz is zw - (z/s) a.lin(du); a stiff row's zw is its dz).
    double dy[NB][3], dwv[6], du[6], dzs_k[NB][9], lrs_k[NB][9];
    auto ZW = [&](int l) -> decltype(auto) { return rst.w(l); };
    // tks_k = W^-1 rz_k - lam \ rsk
    auto tks_of = [&](int k, double* t) {
      double rz[9];
      rzk_of(k, rz);
      winv(k, rz, t);
#pragma unroll
      for (int j = 0; j < 9; ++j) t[j] -= lrs_k[k][j];
    };
    // stiff rows (see the M assembly): the columns H abar_j (core solves with the row's u-space
    // coefficient as bu) and the Cholesky factor of S_ij = a_i . lin(H abar_j) + (s_i / z_i) delta_ij,
    // formed by the predictor's newton call; everything through the lane's scratch record, in run-time
    // loops over the stiff rows (well-scaled QPs never enter)
    const int nst = __builtin_popcount(smask);
    if (nst > 0) out.stiff = 1;
    // a_j . lin(v) of stiff row j
    auto srow = [&](int j, const double* v) -> double {
      const double* r = srec + j * STIFF_ROW;
      double dv2[3], dw2[3];
      lin(v, dv2, dw2);
      const double* x = r[3] != 0.0 ? dw2 : dv2;
      return r[0] * x[0] + r[1] * x[1] + r[2] * x[2];
    };
    // stiff-row step: residuals r_j (in scratch at offset `ro` of each row record) of the stiff rows'
    // equations are turned into dz = S^-1 r (in place), and (yy, ww, uu) += sum_j dz_j H abar_j
    auto stiff_update = [&](int ro, double yy[NB][3], double* ww, double* uu) {
#pragma unroll 1
      for (int i = 0; i < nst; ++i) {
        double t = srec[i * STIFF_ROW + ro];
#pragma unroll 1
        for (int k = 0; k < i; ++k) t -= sfac[i * (i + 1) / 2 + k] * srec[k * STIFF_ROW + ro];
        srec[i * STIFF_ROW + ro] = t * sfac[i * (i + 1) / 2 + i];
      }
#pragma unroll 1
      for (int i = nst - 1; i >= 0; --i) {
        double t = srec[i * STIFF_ROW + ro];
#pragma unroll 1
        for (int k = i + 1; k < nst; ++k) t -= sfac[k * (k + 1) / 2 + i] * srec[k * STIFF_ROW + ro];
        srec[i * STIFF_ROW + ro] = t * sfac[i * (i + 1) / 2 + i];
      }
#pragma unroll 1
      for (int j = 0; j < nst; ++j) {
        const double f = srec[j * STIFF_ROW + ro];
        const double* h = hcol + j * stiff_col(NB);
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
          for (int c = 0; c < 3; ++c) yy[k][c] += f * h[3 * k + c];
#pragma unroll
        for (int q = 0; q < 6; ++q) { ww[q] += f * h[3 * NB + q]; uu[q] += f * h[3 * NB + 6 + q]; }
      }
    };
    // stiff row slot l <-> scratch index j (position among the stiff slots)
    auto spos = [&](int l) -> int { return __builtin_popcount(smask & ((1u << l) - 1u)); };
    auto newton = [&](const double rsk[NB][9], bool corr, const double* ddva, const double* ddwa, double sigmu) {
      double bk[NB][3], bu[6];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        lrs_k[k][0] = rsk[k][0] * frcp(LAM(k, 0));
        {
          double l4[4];
          lam4(k, 1, l4);
          soc_jdiv(l4, rsk[k] + 1, lrs_k[k] + 1);
          lam4(k, 5, l4);
          soc_jdiv(l4, rsk[k] + 5, lrs_k[k] + 5);
        }
        double tks[9], g3[3];
        tks_of(k, tks);
        gs_tmul(k, tks, g3);
#pragma unroll
        for (int c = 0; c < 3; ++c) bk[k][c] = -RK(k, c) - g3[c];
      }
      // stiff rows: right-hand sides g of their equations go to the scratch record (their zw is 0 in bu)
      for_rows([&](int l, const RowRec& rr) {
        const double sl = rr.s, zl = rr.z, bl = rr.b;
        const double* al3 = rr.a;
        const double is = frcp(sl);
        const double rzl = sl - (dot3x(l, al3, dv, dw) + bl);
        const bool stf = (smask >> l) & 1u;
        double cadd = 0.0;
        if (corr) {
          const double a = dot3x(l, al3, ddva, ddwa);
          cadd = act(l) * ((-rzl + a) * (stf ? (double)ZW(l) : ZW(l) - zl * is * a) - sigmu);
        }
        if (__builtin_expect(stf, 0)) {
          srec[spos(l) * STIFF_ROW + 5] = rzl - sl - cadd * frcp(zl);
          ZW(l) = 0.0;
        } else {
          ZW(l) = (zl * rzl - (sl * zl + cadd)) * is;
        }
      });
      rows_adj(ZW, bu);
      if (__builtin_expect(!corr && nst > 0, 0)) {
        // the predictor's call first solves for the iteration's stiff-row columns H abar_j (bk = 0,
        // Rf = 0, bu = abar_j) and factors their Schur complement
        // (k_cadmm_tail: the agent lane's nclone bit-identical clones take every nclone-th column, into the
        // agent's shared scratch record in LDS; the Schur factorisation below reads all of them)
#pragma unroll 1
        for (int j = clone; j < nst; j += nclone) {
          double ab[6];
          {
            const double* r = srec + j * STIFF_ROW;
            double gv[3] = {0, 0, 0}, gw[3] = {0, 0, 0};
            double* g = r[3] != 0.0 ? gw : gv;
            g[0] = r[0]; g[1] = r[1]; g[2] = r[2];
            adj(gv, gw, ab);
          }
          double zb[NB][3], z6[6] = {0, 0, 0, 0, 0, 0}, cy[NB][3], cw[6], cu[6];
#pragma unroll
          for (int k = 0; k < NB; ++k) zb[k][0] = zb[k][1] = zb[k][2] = 0.0;
          core(zb, z6, ab, true, false, cy, cw, cu);
          double* h = hcol + j * stiff_col(NB);
#pragma unroll
          for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) h[3 * k + c] = cy[k][c];
#pragma unroll
          for (int q = 0; q < 6; ++q) { h[3 * NB + q] = cw[q]; h[3 * NB + 6 + q] = cu[q]; }
        }
#if defined(__HIP_DEVICE_COMPILE__)
        if (nclone > 1) {  // the other clones' columns: stores complete before the reads below (one wavefront)
          __builtin_amdgcn_s_waitcnt(0);
          __atomic_signal_fence(__ATOMIC_SEQ_CST);
        }
#endif
        // Cholesky of the symmetrised Schur complement S, column by column
#pragma unroll 1
        for (int j = 0; j < nst; ++j) {
          double d = srow(j, hcol + j * stiff_col(NB) + 3 * NB + 6) + srec[j * STIFF_ROW + 4];
#pragma unroll 1
          for (int k = 0; k < j; ++k) d -= sfac[j * (j + 1) / 2 + k] * sfac[j * (j + 1) / 2 + k];
          const double id = frcp(sqrt(fmax(d, 1e-300)));
          sfac[j * (j + 1) / 2 + j] = id;
#pragma unroll 1
          for (int i = j + 1; i < nst; ++i) {
            double t = 0.5 * (srow(i, hcol + j * stiff_col(NB) + 3 * NB + 6) +
                              srow(j, hcol + i * stiff_col(NB) + 3 * NB + 6));
#pragma unroll 1
            for (int k = 0; k < j; ++k) t -= sfac[i * (i + 1) / 2 + k] * sfac[j * (j + 1) / 2 + k];
            sfac[i * (i + 1) / 2 + j] = t * id;
          }
        }
    }
      {
        double rfv[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) rfv[r] = RF(r);
        core(bk, rfv, bu, true, false, dy, dwv, du);
      }
      // stiff rows' dual directions dz (scratch, and their zw slots)
      auto stiff_store = [&]() {
#pragma unroll
        for (int l = 0; l < NR; ++l)
          if (__builtin_expect((smask >> l) & 1u, 0)) ZW(l) = srec[spos(l) * STIFF_ROW + 6];
      };
      if (__builtin_expect(nst > 0, 0)) {
#pragma unroll 1
        for (int j = 0; j < nst; ++j) srec[j * STIFF_ROW + 6] = srec[j * STIFF_ROW + 5] - srow(j, du);
        stiff_update(6, dy, dwv, du);
        stiff_store();
      }
      // the affine (predictor) direction only sets the step length, sigma and the corrector's
      // second-order term: it is used unrefined; the corrector -- the step actually taken -- is refined
      // (a gate skipping the pass when every row's barrier weight z/s < 1 -- tools/ipm_stats.py: no
      // correction was ever applied below z/s = 10 on the C4 loop -- measured slower: C4 k_cadmm 3.74 ->
      // 4.00 ms, the extra live value costs more than the skipped residual)
      const int nref = corr ? (ROB ? NREF_ROB : NREF) : 0;
      if (corr) DAT_STAT(0);
#pragma unroll 1
      for (int ref = 0; ref < nref; ++ref) {
        DAT_STAT(1);
        ++out.refs;
        if (ref == 1) DAT_STAT_H(2);
        // linearised dual residual of the full system at (dy, dw); refine
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          double tks[9], g9[9];
          tks_of(k, tks);
          gs_mul(k, dy[k], g9);
#pragma unroll
          for (int j = 0; j < 9; ++j) dzs_k[k][j] = tks[j] + g9[j];
        }
        double ddv[3], ddw[3], dpi[6];
        lin(du, ddv, ddw);
        spmv6(Cp(), du, dpi);
        {
          double gv[3] = {0, 0, 0}, gw[3] = {0, 0, 0}, adz[6];
          for_rows([&](int l, const RowRec& rr) {
            const double sl = rr.s, zl = rr.z;
            const double* a = rr.a;
            const bool stf = (smask >> l) & 1u;
            const double dzl = stf ? (double)ZW(l) : ZW(l) - zl * frcp(sl) * dot3x(l, a, ddv, ddw);
            double* g = l < NWROW ? gw : gv;
            g[0] += dzl * a[0]; g[1] += dzl * a[1]; g[2] += dzl * a[2];
          });
          adj(gv, gw, adz);
#pragma unroll
          for (int r = 0; r < 6; ++r) dpi[r] -= adz[r];
        }
        double ek[NB][3], ef[6];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          double ut[3], g3[3];
          Ut_apply(rt.get(k), dpi, ut);
          gs_tmul(k, dzs_k[k], g3);
#pragma unroll
          for (int c = 0; c < 3; ++c) ek[k][c] = -(kap * dy[k][c] + ut[c] + g3[c] + RK(k, c));
        }
        if (MODE == MODE_CADMM) {
          double kp[6];
          Kmul(dpi, kp);
#pragma unroll
          for (int r = 0; r < 6; ++r) ef[r] = P.rho * dwv[r] + kp[r] + RF(r);
        } else if (MODE == MODE_DD) {
#pragma unroll
          for (int r = 0; r < 6; ++r) ef[r] = dpi[r] + RF(r);
        } else {
#pragma unroll
          for (int r = 0; r < 6; ++r) ef[r] = 0.0;
        }
        // stiff rows' equations a_l . lin(du) + (s_l / z_l) dz_l = g_l: their residuals
        double eq = 0.0;
#pragma unroll 1
        for (int j = 0; j < nst; ++j) {
          double* r = srec + j * STIFF_ROW;
          const double q = r[5] - srow(j, du) - r[4] * r[6];
          eq = fmax(eq, fabs(q));
        }
        {  // the linearised system is already solved to rounding: the correction would be noise
           // (stopping here: C4 A/B k_cadmm 11.0 ms with two passes per solve -> 8.9 ms, round 2)
          double en = 0.0, sc = 1.0;
#pragma unroll
          for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) { en = fmax(en, fabs(ek[k][c])); sc = fmax(sc, fabs(RK(k, c))); }
          if constexpr (GRP::on) {
            en = grp.max(en);
            sc = grp.max(sc);
          }
#pragma unroll
          for (int r = 0; r < 6; ++r) { en = fmax(en, fabs(ef[r])); sc = fmax(sc, fabs(RF(r))); }
          en = fmax(en, eq);
#ifdef DAT_IPM_TRACE
          printf("    ref %d en %.3e sc %.3e stiff %d\n", ref, en, sc, nst);
#endif
          if (en <= 1e-12 * sc) {
            DAT_STAT(2);
            if (ref == 0) DAT_STAT_H(0);
            break;
          }

          if (ref == 0) DAT_STAT_H(1);
        }
        ++out.corrs;
        core(ek, ef, nullptr, false, true, dy, dwv, du);
        if (__builtin_expect(nst > 0, 0)) {
          // the stiff-row residuals of the corrected (du, dz), solved into a dz correction (tmp)
#pragma unroll 1
          for (int j = 0; j < nst; ++j) {
            double* r = srec + j * STIFF_ROW;
            r[7] = r[5] - srow(j, du) - r[4] * r[6];
          }
          stiff_update(7, dy, dwv, du);
#pragma unroll 1
          for (int j = 0; j < nst; ++j) srec[j * STIFF_ROW + 6] += srec[j * STIFF_ROW + 7];
          stiff_store();
        }
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        double tks[9], g9[9];
        tks_of(k, tks);
        gs_mul(k, dy[k], g9);
#pragma unroll
        for (int j = 0; j < 9; ++j) dzs_k[k][j] = tks[j] + g9[j];
      }
    };
    // row directions of the current Newton solution
    // (the row's record -- (s, z) pair, coefficients and constant -- was read by the caller's for_rows)
    auto row_dirs = [&](int l, const double* ddv, const double* ddw, const RowRec& rr, double& ds, double& dz) {
      const double sl = rr.s, zl = rr.z, bl = rr.b;
      const double* al3 = rr.a;
      const double a = dot3x(l, al3, ddv, ddw);
      ds = -(sl - (dot3x(l, al3, dv, dw) + bl)) + a;
      dz = ((smask >> l) & 1u) ? (double)ZW(l) : ZW(l) - zl * frcp(sl) * a;
    };
    // step_len / gap_at / the update take the row-space image (ddv, ddw) = lin(du) of the current
    // direction, computed once per direction by the caller
    auto step_len = [&](const double* ddv, const double* ddw) {
      double a = 1e300;
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        double dss[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) dss[j] = -lrs_k[k][j] - dzs_k[k][j];
        const double l0 = LAM(k, 0);
        if (dss[0] < 0) a = fmin(a, -l0 * frcp(dss[0]));
        if (dzs_k[k][0] < 0) a = fmin(a, -l0 * frcp(dzs_k[k][0]));
        double l4[4];
        lam4(k, 1, l4);
        a = fmin(a, soc_step(l4, dss + 1));
        a = fmin(a, soc_step(l4, dzs_k[k] + 1));
        lam4(k, 5, l4);
        a = fmin(a, soc_step(l4, dss + 5));
        a = fmin(a, soc_step(l4, dzs_k[k] + 5));
      }
      if constexpr (GRP::on) a = grp.min(a);
      for_rows([&](int l, const RowRec& rr) {
        double ds, dz;
        const double sl = rr.s, zl = rr.z;
        row_dirs(l, ddv, ddw, rr, ds, dz);
        if (ds < 0) a = fmin(a, -sl * frcp(ds));
        if (dz < 0) a = fmin(a, -zl * frcp(dz));
      });
      return a;
    };
    auto gap_at = [&](double al, const double* ddv, const double* ddw) {
      double g = 0.0;
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          double dss = -lrs_k[k][j] - dzs_k[k][j];
          const double lj = LAM(k, j);
          g += (lj + al * dss) * (lj + al * dzs_k[k][j]);
        }
      if constexpr (GRP::on) g = grp.sum(g);
      for_rows([&](int l, const RowRec& rr) {
        double ds, dz;
        const double sl = rr.s, zl = rr.z;
        row_dirs(l, ddv, ddw, rr, ds, dz);
        g += (sl + al * ds) * (zl + al * dz);
      });
      return g;
    };

    // the second-order cones' part of rs = lam o lam of block k (the predictor's and the corrector's targets)
    auto lam_sq = [&](int k, double* rs) {
      double l4[4];
      lam4(k, 1, l4);
      soc_jprod(l4, l4, rs + 1);
      lam4(k, 5, l4);
      soc_jprod(l4, l4, rs + 5);
    };
    // predictor
    DAT_PHASE(4);
    {
      double rsk[NB][9];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const double l0 = LAM(k, 0);
        rsk[k][0] = l0 * l0;
        lam_sq(k, rsk[k]);
      }
      newton(rsk, false, nullptr, nullptr, 0.0);
    }
    {
      DAT_PHASE(5);
      double ddva[3], ddwa[3];  // lin(du) of the affine direction: its step, gap and the corrector's term
      lin(du, ddva, ddwa);
      const double aaff = fmin(1.0, step_len(ddva, ddwa));
      const double gaff = gap_at(aaff, ddva, ddwa);
      double sig = gaff / gap;
      sig = fmax(0.0, fmin(1.0, sig * sig * sig));
      const double sigmu = sig * gap * ideg;
      // corrector: rs = lam o lam + dss_aff o dzs_aff - sig mu e
      double rsk[NB][9];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        double dss[9], c1[4], c2[4];
#pragma unroll
        for (int j = 0; j < 9; ++j) dss[j] = -lrs_k[k][j] - dzs_k[k][j];
        const double l0 = LAM(k, 0);
        rsk[k][0] = l0 * l0 + dss[0] * dzs_k[k][0] - sigmu;
        lam_sq(k, rsk[k]);
        soc_jprod(dss + 1, dzs_k[k] + 1, c1);
        soc_jprod(dss + 5, dzs_k[k] + 5, c2);
#pragma unroll
        for (int j = 0; j < 4; ++j) { rsk[k][1 + j] += c1[j]; rsk[k][5 + j] += c2[j]; }
        rsk[k][1] -= sigmu;
        rsk[k][5] -= sigmu;
      }
      DAT_PHASE(6);
      newton(rsk, true, ddva, ddwa, sigmu);
    }
    DAT_PHASE(7);
    double ddv[3], ddw[3];  // lin(du) of the corrector direction
    lin(du, ddv, ddw);
    double alpha = fmin(1.0, ETA * step_len(ddv, ddw));
    // safeguard: Mehrotra's corrector can increase the gap of a feasible iterate (it then cycles);
    // backtrack until the complementarity gap decreases
    const bool feasible = pres < 1e-8 * NH() && dres < 1e-8 * NQ();
    for (int bt = 0; feasible && bt < 8; ++bt) {
      if (gap_at(alpha, ddv, ddw) <= gap * (1.0 - 0.01 * alpha)) break;
      alpha *= 0.5;
    }
    // update.  ds from the primal equation (keeps G y + s = h exact), dz = W^-1 dzs.
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      double g[9], dz[9], rz[9];
      Gy(dy[k], g);
      winv(k, dzs_k[k], dz);
      rzk_of(k, rz);
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        sk[k][j] = sk[k][j] + alpha * (-rz[j] - g[j]);
        zk[k][j] = zk[k][j] + alpha * dz[j];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) y[k][c] = y[k][c] + alpha * dy[k][c];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) w[r] = w[r] + alpha * dwv[r];
    // (slot l + 1's pair is read before slot l's is written: another slot)
    for_rows([&](int l, const RowRec& rr) {
      double ds, dz;
      const double sl = rr.s, zl = rr.z;
      row_dirs(l, ddv, ddw, rr, ds, dz);
      rst.set_sz(l, sl + alpha * ds, zl + alpha * dz);
    });
  }
  DAT_PHASE(8);
  DAT_STAT(3 + (out.why < 7 ? out.why : 6));
  // not converged to tol: return the best iterate seen; "optimal" if its scaled primal / dual
  // residuals are within north_star's 1e-7 and its complementarity gap within 1e-6 (strongly graded
  // problems -- the rigid payload's Jl^-1 ~ 50 -- can stall at a 1e-7 gap while the structured Newton
  // solve loses accuracy; the minimiser is then still within ~1e-7 of the oracle's), otherwise
  // inaccurate (the reference holds its previous solution).
  if (BK() < 1e300) {
    record();  // the last iterate of an in-band exit: a start for the next pass all the same
#pragma unroll
    for (int k = 0; k < NB; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) y[k][c] = best[3 * k + c];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      w[r] = best[3 * NB + r];
      out.pi[r] = best[3 * NB + 6 + r];
      out.u[r] = best[3 * NB + 12 + r];
    }
    out.status = ST_OPTIMAL;
    out.inband = 1;
    out.merit = BK();
  }
  return out;
}

// The reduced QP solve (ipm_attempt).  A C-ADMM agent QP on the tuned start (P.tuned: the warm closed
// loop) that does not converge to tolerance -- diverged, hit max_iter or stalled -- is solved again from
// the conservative start: with consensus multipliers ~1e2-1e3 (the first, cold steps of C5 / C2, a
// stalled ADMM loop) the tuned start's small duals and 0.999 step fraction can stall (full-size C5 on the
// CPU replica, diag/c5_cpu.py: 153 of 29.2 M agent QPs, 2 of them beyond 1e-8; every one of them
// converges from the conservative start in 7-16 iterations).
//
// ROBUST selects the instantiation.  The robust one carries the stiff-row machinery, which cost k_cadmm's fast
// path 36-60 % when compiled into the same kernel (register allocation, C4 A/B), and so does any test for stiff
// rows inside the fast one (7-14 %): a solve is judged by its outcome instead.  A fast solve that does not
// end cleanly -- not converged to tolerance (INACCURATE), or accepted through an in-band iterate -- is the
// symptom of stiff rows (a stalled ADMM loop's agent QPs, barrier weights 1e10-1e19, whose Newton systems
// lose the digits convergence needs) and is redone by the robust instantiation from scratch; the better of
// the two outcomes is kept (ipm_rank).  A clean fast solve meets the tolerance on residuals evaluated from
// the iterate itself, however its Newton systems were solved.
//   IPM_FAST        fast (k_cadmm, which hands a scenario with an unclean solve to k_cadmm_tail; DD, centralized)
//   IPM_ROBUST      robust
//   IPM_FAST_REDO   the C-ADMM agent QP's definition: fast, redone robustly when not clean (k_cadmm_tail, the
//                   single-QP surfaces, host builds)
//   IPM_FAST_R      IPM_FAST as IPM_FAST_REDO's first attempt: the same arithmetic as a template instance of
//                   its own, so that k_cadmm's IPM_FAST instance has one call site per class and is inlined
//                   (shared with k_cadmm_tail's redo it was called, and k_cadmm took 7 % longer)
enum { IPM_FAST = 0, IPM_FAST_R = 1, IPM_ROBUST = 2, IPM_FAST_REDO = 3 };
// 0 converged, 1 in-band OPTIMAL, 2 not OPTIMAL
DAT_HD int ipm_rank(const IPMOut& r) { return r.status != ST_OPTIMAL ? 2 : r.inband ? 1 : 0; }
// a fast solve k_cadmm hands over (IPM_FAST_REDO redoes it): INACCURATE (not the solver-exception branch,
// ST_FAILED: non-finite data), or accepted through an in-band iterate outside Clarabel's own tolerance (an
// in-band accept within it is one Clarabel would return as well)
DAT_HD bool ipm_unclean(const IPMOut& r) {
  return r.status == ST_INACCURATE || (r.status == ST_OPTIMAL && r.inband && r.merit > IPM_CLARABEL_TOL);
}
template <int MODE, int NB, int NR, class SH, class ER, class RT, class RW = RowRegs, unsigned AUXM = 0,
          class GRP = NoGrp, int ROBUST = IPM_FAST, bool WS = false>
DAT_HD IPMOut ipm_solve(const SH& sh, const ER& er, const RT& rt, const QPLane<NB>& P, const double* y0,
                        double y[NB][3], double w[6], double* best, int max_iter, double tol, RW rw = RW{},
                        GRP grp = GRP{}, double* wrec = nullptr, bool wson = false, int clone = 0, int nclone = 1) {
  if constexpr (ROBUST == IPM_FAST_REDO) {
    // trip 0 fast; trip 1 robust (the fast outcome not clean); trip 2 fast once more when the robust outcome
    // is worse (deterministic: it reproduces the first; keeping the first iterate instead would hold another
    // y, w, pi, u live across the robust solve).  One call site per instantiation (ipm_attempt is inlined
    // into each: an instance called from two sites is compiled out of line, which cost k_cadmm 7 %).
    // WS: trip 0 may start warm (the record's flag); trip 2 restores the flag so that it reproduces trip 0.
    IPMOut o, f;
    int done = 0, done_refs = 0, done_corrs = 0;
    const double wflag = (WS && wrec) ? wrec[0] : 0.0;
#pragma unroll 1
    for (int trip = 0;; ++trip) {
      if (WS && wrec && trip == 2) wrec[0] = wflag;
      if (trip == 1 || (wson && wflag == 1.0))  // a warm first trip (and its rerun, trip 2) runs the robust solver
        o = ipm_solve<MODE, NB, NR, SH, ER, RT, RW, AUXM, GRP, IPM_ROBUST, WS>(sh, er, rt, P, y0, y, w, best, max_iter,
                                                                               tol, rw, grp, wrec, wson, clone, nclone);
      else
        o = ipm_solve<MODE, NB, NR, SH, ER, RT, RW, AUXM, GRP, IPM_FAST_R, WS>(sh, er, rt, P, y0, y, w, best, max_iter,
                                                                               tol, rw, grp, wrec, wson, clone, nclone);
      o.iters += done;
      o.refs += done_refs;
      o.corrs += done_corrs;
      if (trip == 2) break;
      if (trip == 0) {
        if (!ipm_unclean(o)) return o;
        f = o;
      } else {
        const int rf = ipm_rank(f), rr = ipm_rank(o);
        if (!(rr > rf || (rr == rf && rr == 1 && o.merit > f.merit))) break;
      }
      done = o.iters;
      done_refs = o.refs;
      done_corrs = o.corrs;
    }
    o.stiff = 1;  // redone robustly
    return o;
  } else {
    constexpr bool ROB = ROBUST == IPM_ROBUST;
    // First start: tuned for the C-ADMM agent QPs of the warm closed loop (P.tuned), conservative otherwise.
    // A tuned attempt that does not converge cleanly is redone from the conservative start (a tuned attempt
    // that has not converged in 20 iterations is not converging: C4's tuned solves take 4.3 on average and
    // at most ~10).  A conservative attempt accepted through an in-band iterate outside Clarabel's 1e-8
    // (rounding-path accidents, ~1 agent QP in 10^7 on C5 and C1: the same QPs on the host build converge
    // from either start) is redone from another start (C-ADMM: tuned; DD / centralized: the conservative
    // start scaled by 10), whose result is taken unless it is worse than the first: then the first start
    // is run once more (the attempts are deterministic, so that reproduces the first result; keeping it in
    // registers instead cost k_cadmm 4 % and k_cent 50 % in register pressure, round 4).  (Not the attempts
    // that end with no in-band iterate: they already ran to max_iter, and a second 50 iterations lengthened
    // C1's slowest wavefront by 45 %.)  One code instance runs every attempt (unroll 1).
    const int first = MODE == MODE_CADMM && P.tuned ? 1 : 0;
    int start = first, trip = 0, done = 0, done_refs = 0, done_corrs = 0;
    int rank0 = 0;  // first attempt: 0 converged, 1 in-band OPTIMAL, 2 not OPTIMAL
    double merit0 = 0.0;
    IPMOut o;
    if constexpr (WS) {
      if (wson && wrec && wrec[0] == 1.0) start = 3;  // the warm attempt first (a converged previous pass)
    }
#pragma unroll 1
    for (;;) {
      // (the tuned start as the first attempt is capped at 20 iterations: see above; the warm one at WS_MAXIT)
      o = ipm_attempt<MODE, NB, NR, SH, ER, RT, RW, AUXM, GRP, ROB, WS>(
          sh, er, rt, P, y0, y, w, best,
          start == 3 ? (max_iter > WS_MAXIT ? WS_MAXIT : max_iter)
                     : start == 1 && trip != 1 && max_iter > 20 ? 20 : max_iter,
          tol, rw, grp, start, wrec, wson, clone, nclone);
      o.iters += done;
      o.refs += done_refs;
      o.corrs += done_corrs;
      if (WS && start == 3) {
        // the warm attempt: converged cleanly, stalled in band within WS_STALL_TOL (or certified), else the cold
        // sequence from its first start
        if ((o.why == 0 && !o.inband) || o.why == 7 || o.status == ST_FAILED || o.status == ST_INFEASIBLE) break;
        start = first;
        done = o.iters;
        done_refs = o.refs;
        done_corrs = o.corrs;
        continue;
      }
      if (trip == 2) break;
      if (trip == 1) {
        const int r1 = ipm_rank(o);
        if (r1 < rank0 || (r1 == rank0 && (r1 != 1 || o.merit <= merit0))) break;
        start = first;  // the second attempt is worse: redo the first
      } else {
        if (o.status == ST_FAILED || o.status == ST_INFEASIBLE) break;
        if (start == 1) {
          if ((o.why == 0 && !o.inband) || (WS && o.why == 7)) break;
          start = 0;
        } else {
          if (!(o.status == ST_OPTIMAL && o.inband && o.merit > IPM_CLARABEL_TOL)) break;
          start = MODE == MODE_CADMM ? 1 : 2;
        }
        rank0 = ipm_rank(o);
        merit0 = o.merit;
      }
      ++trip;
      done = o.iters;
      done_refs = o.refs;
      done_corrs = o.corrs;
    }
    if constexpr (WS) {  // only an OPTIMAL solve (converged or in band) leaves a warm start for the next pass
      if (wrec && o.status != ST_OPTIMAL) wrec[0] = 0.0;
    }
    return o;
  }
}

// Solve with the smallest row-slot instantiation that covers every lane of the wavefront
// (nr_wave: wave-uniform maximum of rows_needed over the lanes taking part).
template <int MODE, int NB, int ROBUST = IPM_FAST, bool WS = false, class SH, class ER, class RT>
DAT_HD IPMOut ipm_solve_rows(int nr_wave, const SH& sh, const ER& er, const RT& rt, const QPLane<NB>& P,
                             const double* y0, double y[NB][3], double w[6], double* best, int max_iter, double tol,
                             double* wrec = nullptr, bool wson = false) {
  if (nr_wave <= NBASE)
    return ipm_solve<MODE, NB, NBASE, SH, ER, RT, RowRegs, 0, NoGrp, ROBUST, WS>(sh, er, rt, P, y0, y, w, best,
                                                                                 max_iter, tol, RowRegs{}, NoGrp{}, wrec, wson);
  return ipm_solve<MODE, NB, DAT_MAXROW, SH, ER, RT, RowRegs, 0, NoGrp, ROBUST, WS>(sh, er, rt, P, y0, y, w, best,
                                                                                    max_iter, tol, RowRegs{}, NoGrp{},
                                                                                    wrec, wson);
}

}  // namespace dat
