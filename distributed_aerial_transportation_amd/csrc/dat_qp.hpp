// dat_qp.hpp -- the reduced agent QP (per-lane fp64 device code): the constants, the QP's data (QPShared, EnvRows,
// the accessors, QPLane, build_shared, set_env_rows, dvl_rows_infeasible, lane_*) and, included at the end, its
// interior-point solver (dat_ipm.hpp).  This is the include everyone uses.
//
// Data placement (DESIGN.md "Register and LDS budget"):
//   QPShared   everything that is the same for all agents of one scenario (u-maps, the packed
//              u-space Hessians, the base rows, the C-ADMM aggregate K).  The C-ADMM / DD kernels
//              keep one copy per scenario in LDS; the centralized kernel keeps it in registers.
//   EnvRows    the agent's env CBF rows (LDS in the C-ADMM / DD kernels).
//   Rt         the agent's U-map hat(r_com) Rl' (LDS in the C-ADMM / DD kernels), read through an
//              accessor at each use.
//   QPLane     the agent's per-solve scalars and linear terms (registers).
//   best       the best iterate seen (lane-private global memory: written, read only on failure).
// Every array the solver keeps in registers is indexed with compile-time indices only (rows are
// fixed slots with an activity mask, loops are unrolled, the LU row exchange is a predicated
// swap), so nothing is demoted to scratch memory.
//
// u = (S, Mo) in R^6: aggregate force and moment about the CoM in payload axes,
//   S = sum_j f_j,  Mo = sum_j hat(r_com_j) Rl' f_j      (control/rqp_cadmm.py:376-392)
// Accelerations are affine in u:
//   dwl = JT^-1 Mo + bw,           bw = -JT^-1 (wl x JT wl)
//   dvl = S/mT + Bv Mo + bv,       Bv = Rl hat(x_com) JT^-1,
//                                  bv = -g e3 - Rl hat(wl)^2 x_com + Rl hat(x_com) bw
// Cone block k (an agent's own force f_k in R^3): f_kz >= min_fz, ||f_k|| <= sec f_kz,
// ||f_k|| <= max_f.  Row slots (affine in (dvl, dwl)):  0 tilt (dwl), 1 |wl| (dwl), 2 |vl| (dvl),
// 3 .. 3+DAT_NENV-1 env CBFs (dvl).  Active env rows are compacted to the front of the env
// slots, so a solve whose rows all fit in NR slots runs the NR-slot instantiation.
#pragma once

#include "dat_core.hpp"

namespace dat {

constexpr int NWROW = 2;          // slots [0, NWROW) act on dwl
constexpr int NBASE = 3;          // base slots shared by all agents of a scenario
// iterative-refinement passes per corrector solve (at most; a pass stops the loop once the linearised
// system is solved to rounding, so well-scaled QPs run one).  Badly scaled agent QPs -- consensus
// multipliers ~1e3-1e4 in a stalled ADMM loop, active rows with barrier weights z/s ~1e15 -- need up to
// six to keep the dual residual below the stopping tolerance (tools/hard_qp_probe.py: 2 passes left
// 281 of 798 such solves at in-band exits, 6 passes 69, all within 1.5e-6 of the oracle)
constexpr int NREF = 6;
// The robust instantiation (stiff rows in augmented form) at most one: on the C4 stall stretches (host build,
// tools/stall_warm_hostsim.py) its warm-started solves ran 4.75 refinement passes and 4.43 corrections per IPM
// iteration with six -- most stop at the cap, the residual of the augmented system does not reach the rounding
// test -- 1.9 / 1.7 with two and 1.0 / 0.9 with one, at about the same IPM iterations per solve (8.5, 8.2) and
// f_des within 1.5e-6 of the oracle.  GPU A/B (tools/r06_ab.sh): the stall stretches alone 48.1 / 36.5 -> 41.6 /
// 33.2 ms per step, the 10 s loop 36.0 -> 33.0 ms per step on average, 0 accepts beyond 1e-8 either way.
constexpr int NREF_ROB = 1;
// Initial point: cone / row slacks shifted to at least IPM_S0 inside, duals IPM_Z0 e.  The agent QPs'
// multipliers are O(1e-2) at the solution; starting the duals and the slack margins there instead of at 1
// takes 7.00 -> 5.23 IPM iterations per C-ADMM agent QP on the C4 closed loop (CPU sweep over
// {0.01, 0.03, 0.1, 0.3, 1, 3, 10}^2, tools/ipm_init_sweep.py; same solutions to the solver tolerance).
constexpr double IPM_S0 = 0.03, IPM_Z0 = 0.03;
constexpr double IPM_ETA = 0.999;  // fraction of the step to the cone boundary (7.00 -> 5.23 -> 4.28 it/QP)
// DD agent QPs: the conservative start.  Round-3 A/B on C3 (IPM it/QP, ms per step against 9.46,
// 20.3 / 20.7): S0 = Z0 = 0.3 -> 9.00, 21.4; 0.1 -> 8.89, 22.0; ETA 0.995 -> 9.29, 20.9; 0.1 and 0.995 ->
// 8.71, 21.8 -- fewer iterations on average, a wider spread across a wavefront.
constexpr double DD_S0 = 1.0, DD_Z0 = 1.0, DD_ETA = 0.99;
// divergence stop (from the 5th iteration): merit above IPM_DIVERGE x the best seen.  A start close to
// the boundary can raise the residuals by 1e3 in its first steps on a well-posed DD QP.
constexpr double IPM_DIVERGE = 1e6;

// Every array starts on a 16-byte boundary and the kernels place the record 16-byte aligned in LDS,
// so the solver reads entry pairs (ldn: one ds_read_b128 per pair).
struct alignas(16) QPShared {
  double C[2][22];       // packed u-space Hessian (21 + pad): [0] without, [1] with the leader's desired-acc terms
  double K[22];          // C-ADMM: sum over ALL agents of U_j U_j' (agent i subtracts its own term)
  double cu[2][6];       // matching linear terms
  double Bv[10], JTi[10];  // 3x3 row-major + pad
  double rows[NBASE][4]; // base rows (a0, a1, a2, b): coefficients on dwl (slots 0, 1) or dvl (slot 2) and
                         // the constant (the affine offsets bw / bv folded in)
  double bv[4], bw[4];
  double inv_mT, pad_;
  int bmask;             // active base slots
  int infeasible;        // a dropped all-zero row had a negative constant
  int pad2_[2];
};
// LDS stride (doubles) of the U-maps Rt_j the C-ADMM / DD kernels keep per agent: 9 + pad, so each
// map starts on a 16-byte boundary (ldn pair reads)
constexpr int RT_STRIDE = 10;

// env CBF rows of one agent (dvl): a . lin_v(u) + b >= 0 (kept in LDS by the kernels)
struct EnvRows {
  double a[DAT_NENV][3], b[DAT_NENV];
};

// Access to solver data kept outside the register file.  get() re-derives the reference through
// an index the compiler cannot see through, so loads are issued where the data is consumed and
// never hoisted out of the IPM loop or merged across uses (hoisting would pin ~150 doubles of
// loop-invariant data in registers and spill the iterates).
template <class T>
struct PlainRef {
  const T* p;
  DAT_HD const T& get() const { return *p; }
};
// LDS records are read through volatile address_space(3) pointers computed once, outside the
// solver loops: every use is a ds_read with an immediate offset at the point of use (the compiler
// may not hoist, merge or cache a volatile load), costing no register between uses and no address
// arithmetic.
template <class T>
__device__ inline const DAT_LDS T* lds_opaque(const DAT_LDS T* p) {
  __asm__ volatile("" : "+v"(p));
  return p;
}
template <class T>
struct LdsRef {
  const volatile DAT_LDS T* p;
  __device__ LdsRef(const T* b, int idx) : p((const volatile DAT_LDS T*)(b + idx)) {}
  __device__ const volatile DAT_LDS T& get() const { return *p; }
};
// env-row accessors: a(j, c), b(j) of env slot j
struct EnvPlain {
  const EnvRows* p;
  DAT_HD double a(int j, int c) const { return p->a[j][c]; }
  DAT_HD double b(int j) const { return p->b[j]; }
  DAT_HD void a3(int j, double* o) const { o[0] = p->a[j][0]; o[1] = p->a[j][1]; o[2] = p->a[j][2]; }
  DAT_HD void ab(int j, double* o, double& bb) const { a3(j, o); bb = p->b[j]; }
};
// LDS image of the env rows of a 64-lane wavefront, pairs structure of arrays: env slot j is two
// pair fields, (a_j0, a_j1) and (a_j2, b_j), each 64 lanes x 16 bytes, so a lane reads a row with two
// ds_read_b128 and a wavefront reading one field touches 1 KB of consecutive LDS (conflict free):
//   field 2 j + h of lane l at doubles [(2 j + h) * 128 + 2 l, +1].
__host__ __device__ constexpr int env_lds_doubles(int NE) { return 4 * NE * 64; }
constexpr int ENV_LDS_DOUBLES = env_lds_doubles(DAT_NENV);
DAT_HD constexpr int env_lds_index(int j, int c, int lane) { return (2 * j + (c >> 1)) * 128 + 2 * lane + (c & 1); }
template <int NE>
struct EnvLdsN {
  const DAT_LDS double* p;  // the lane's pair column
  __device__ EnvLdsN(const double* b, int lane) : p((const DAT_LDS double*)(b + 2 * lane)) {}
  __device__ dat_d2 field(int f) const { return ((const volatile DAT_LDS dat_d2*)p)[f * 64]; }
  __device__ double a(int j, int c) const { return ((const volatile DAT_LDS double*)p)[env_lds_index(j, c, 0)]; }
  __device__ double b(int j) const { return ((const volatile DAT_LDS double*)p)[env_lds_index(j, 3, 0)]; }
  __device__ void a3(int j, double* o) const {
    const dat_d2 f0 = field(2 * j), f1 = field(2 * j + 1);
    o[0] = f0.x; o[1] = f0.y; o[2] = f1.x;
  }
  __device__ void ab(int j, double* o, double& bb) const {
    const dat_d2 f0 = field(2 * j), f1 = field(2 * j + 1);
    o[0] = f0.x; o[1] = f0.y; o[2] = f1.x;
    bb = f1.y;
  }
};
using EnvLds = EnvLdsN<DAT_NENV>;
// the first NE slots of E (set_env_rows compacts the active rows to the front)
template <int NE = DAT_NENV>
DAT_HD void env_to_lds(double* base, int lane, const EnvRows& E) {
#pragma unroll
  for (int j = 0; j < NE; ++j) {
#pragma unroll
    for (int c = 0; c < 3; ++c) base[env_lds_index(j, c, lane)] = E.a[j][c];
    base[env_lds_index(j, 3, lane)] = E.b[j];
  }
}

// U-map accessors: get(k) -> Rt_k (9 doubles, row-major) of cone block k
struct RtPtr {
  const double* p;  // NB x 9
  DAT_HD const double* get(int k) const { return p + 9 * k; }
};
struct RtLds {
  const volatile DAT_LDS double* p;  // block 0
  __device__ RtLds(const double* b, int off) : p((const volatile DAT_LDS double*)(b + off)) {}
  __device__ const volatile DAT_LDS double* get(int k) const { return p + RT_STRIDE * k; }
};

template <int NB>
struct QPLane {
  int var;                       // C / cu variant
  unsigned emask;                // active env slots (compacted: bits 0 .. k-1)
  int infeasible;
  int tuned;                     // C-ADMM: first ADMM pass of the step (tuned IPM start, see ipm_solve)
  double kappa, rho, min_fz, max_f, sec;
  double a2;                     // C-ADMM: sum_{j != i} ||a_j||^2 (objective constant of the free blocks)
  double q[NB][3];               // per-block linear term
  double atil[6];                // C-ADMM: sum_{j != i} U_j a_j
  double cw[6];                  // DD: linear cost on w = (F_i, M_i)
};

// row slots an IPM instantiation must cover for a lane whose env mask is emask
DAT_HD int rows_needed(unsigned emask) { return NBASE + (emask ? 32 - __builtin_clz(emask) : 0); }

// Stiff rows: a row slot whose barrier weight z/s exceeds IPM_STIFF_W is kept out of the normal-equation
// matrix M and solved in augmented (quasi-definite) form, at most IPM_NSTIFF per solve (see ipm_attempt)
constexpr double IPM_STIFF_W = 1e12;
constexpr int IPM_NSTIFF = 8;

// size (doubles) of the lane-private best-iterate record: y (3 NB), w (6), pi (6), u (6) (best_rec: all a
// non-robust instantiation touches, the stride k_cadmm, DD and centralized index with) plus, behind it, the
// robust instantiation's stiff-row scratch of an iteration (ipm_attempt): per stiff row j a column
// H abar_j = (dy (3 NB), dw (6), du (6)), the row (a (3), on-dwl flag, s / z), its right-hand side g and
// dual direction dz (and a temporary); the Cholesky factor of the Schur complement (packed lower, reciprocal diagonal)
DAT_HD constexpr int best_rec(int NB) { return 3 * NB + 18; }
DAT_HD constexpr int stiff_col(int NB) { return 3 * NB + 12; }
constexpr int STIFF_ROW = 8;  // a0 a1 a2 on_dwl e g dz tmp
// (and, last, FM_DOUBLES for the warm-start instantiation's u-space factor P: ipm_attempt WS)
constexpr int FM_DOUBLES = 21;
DAT_HD constexpr int best_size(int NB) {
  return best_rec(NB) + IPM_NSTIFF * (stiff_col(NB) + STIFF_ROW) + IPM_NSTIFF * (IPM_NSTIFF + 1) / 2 + FM_DOUBLES;
}
// Clarabel's own tolerance: an in-band exit whose merit is above it is one Clarabel would not certify
constexpr double IPM_CLARABEL_TOL = 1e-8;
// the IPM's iteration cap and default stopping tolerance (dat_set_qp_tolerance), for the kernels and the host step
constexpr int IPM_MAX_ITER = 50;
constexpr double IPM_TOL = 1e-10;

// Warm start (start 3, ipm_solve WS): the previous ADMM pass's last iterate of the same agent QP (of a converged,
// stall-exited or in-band OPTIMAL solve), in a lane record of WREC_SIZE doubles -- [0] valid flag, y (3), w (6),
// cone slacks (9) and duals (9), the row slacks and duals (DAT_MAXROW each) -- pushed back into the interior so
// that every complementarity pair's product is at least WS_MU (a pair (s, z) below it moves to (s + d, z + d); a
// second-order cone pair by its margins s0 - |s1:3|, z0 - |z1:3|), and solved by the robust instantiation (the
// stall's active rows carry barrier weights of 1e10 and more from the first iteration).  The attempt is capped at
// WS_MAXIT iterations; one that does not end cleanly goes on to the cold starts.  Host build, C4 stall stretches
// (2 x 20 HL steps of 101-pass stalls, tools/stall_warm_hostsim.py): the critical path (the slowest agent QP of
// every pass) 25-32 IPM iterations per pass cold, ~10 warm; f_des within 2.2e-6 of the oracle where it is
// reproducible.  WS_MU in 1e-2 .. 1e3 measured alike (42-49 k critical iterations over the stretches); 1e2 has
// the smallest f_des difference.
constexpr double WS_MU = 1e2;
constexpr int WS_MAXIT = 30;
// the DD agent QPs' warm-start floor (dat.hip DD_WARM_PASS): better scaled than a stalled C-ADMM loop's, they take
// a far smaller push (C3: 1e2 19.0, 1e0 14.0, 1e-2 11.2, 1e-3 10.7, 1e-4 11.0 ms per step warm from pass 1)
constexpr double DD_WS_MU = 1e-3;
// stall exit of the tail kernel's solves (ipm_attempt WS): best in-band merit <= WS_STALL_TOL and not halved
// in WS_STALL_ITS iterations
constexpr double WS_STALL_TOL = 1e-9;
// (WS_STALL_ITS 3 -> 2: stall fixture 39.7 / 30.1 -> 37.7 / 29.5 ms per stalled step, same-call A/B, f_des and ADMM
// counts against the oracle unchanged.  1 measured 35.4 / 29.1 but left the host build of the second stall stretch
// 3.2e-5 off the oracle at step 5, beyond its 1.8e-5 bound (test_hostsim); WS_STALL_TOL 3e-9 and WS_MAXIT 15 measured
// no faster)
constexpr int WS_STALL_ITS = 2;
constexpr int WREC_SIZE = 28 + 2 * DAT_MAXROW;
// The tail rule of the C-ADMM closed loop with a forest: ADMM pass p of a scenario's control step solves its
// agent QPs with the warm start and the stall exit exactly when p >= 1 and (the scenario's previous step took more
// than TAIL_PREV passes -- it is wedged in a stall, where every step is the reference loop's 101-pass max_iter
// stall, control/rqp_cadmm.py:661 -- or p >= TAIL_PASS).  The GPU runs those passes in k_cadmm_tail (dat_k_cadmm_tail.hip).
// The rule depends on the scenario's own history only, so its results do not depend on the scenarios it is
// batched with.  Normal C4 steps take 1-14 passes: the warm closed loop never meets it.
// (TAIL_PASS = 8 measured worse: the warm window's 9-14-pass scenarios then finish after k_cadmm, C4 3.87 -> 4.58
// ms per step, and the 10 s loop did not gain, 33.0 -> 34.0 ms per step; tools/r06_ab.sh)
// The rule as predicates (tail_rule, tail_wedged): dat_cadmm_step.hpp.
constexpr int TAIL_PREV = 20, TAIL_PASS = 16;

// ------------------------------------------------------------------ shared data
// k_f, k_m: total force / moment weights; variants: bit 0 build C[0] (kdv = 0), bit 1 build C[1]
// (kdv = 1).  with_K: C-ADMM aggregate over all agents.
// build_shared_inl is the text, inlined where it stands: the C-ADMM drains build at one site (cadmm_drain: a slot's new
// scenario and a fused next step both go through the top of the pass), so their kernels hold no call -- a call in
// the persistent loop makes the register allocator save and restore the drain's state around it.  build_shared is
// the same text out of line, for the callers with more than one site (the DD drain: a new scenario, and a fused
// next step) and the host builds: one compiled body keeps a unit's sites bitwise identical.  -ffp-contract=on fuses
// multiply-adds within an expression only, so the inlined and the out-of-line text compute the same bits.
__host__ __device__ inline __attribute__((always_inline)) void build_shared_inl(QPShared& S, const double* prm, int n,
                                                                                 const double* st, const double* acc,
                                                                                 double k_f, double k_m, int variants,
                                                                                 bool with_K) {
  const double mT = prm[DAT_P_MT];
  const double* xc = prm + DAT_P_XCOM;
  const double* JT = prm + DAT_P_JT;
  const double* JTi = prm + DAT_P_JTI;
  const double* Rl = st + DAT_S_RL(n);
  const double* wl = st + DAT_S_WL(n);
  const double* vl = st + DAT_S_VL(n);
  S.inv_mT = 1.0 / mT;
  for (int i = 0; i < 9; ++i) S.JTi[i] = JTi[i];
  double Xh[9], RX[9];
  skew3(xc, Xh);
  mm3(Rl, Xh, RX);              // Rl hat(x_com)
  mm3(RX, JTi, S.Bv);           // Rl hat(x_com) JT^-1
  double Jw[3], wJw[3], bw[3], bv[3];
  mv3(JT, wl, Jw);
  cross3(wl, Jw, wJw);
  mv3(JTi, wJw, bw);            // c_w = JT^-1 (wl x JT wl)
  bw[0] = -bw[0]; bw[1] = -bw[1]; bw[2] = -bw[2];
  // bv = -g e3 - Rl hat(wl)^2 x_com + Rl hat(x_com) bw
  double wx[3], wwx[3], t1[3], t2[3];
  cross3(wl, xc, wx);
  cross3(wl, wx, wwx);
  mv3(Rl, wwx, t1);
  mv3(RX, bw, t2);
  bv[0] = -t1[0] + t2[0];
  bv[1] = -t1[1] + t2[1];
  bv[2] = -DAT_GRAVITY - t1[2] + t2[2];
  for (int c = 0; c < 3; ++c) { S.bw[c] = bw[c]; S.bv[c] = bv[c]; }
  S.bw[3] = S.bv[3] = 0.0;
  S.Bv[9] = S.JTi[9] = 0.0;
  S.pad_ = 0.0;

  // Phi(u) = k_f ||S - mT g e3||^2 + k_m ||Mo||^2 + kdv (||dvl||^2 - 2 dvl_des'dvl)
  //          + kdv (||dwl||^2 - 2 dwl_des'dwl)          (control/rqp_cadmm.py:436-458)
  for (int v = 0; v < 2; ++v) {
    if (!((variants >> v) & 1)) continue;
    double* C = S.C[v];
    double* cu = S.cu[v];
    for (int k = 0; k < 22; ++k) C[k] = 0.0;
    for (int r = 0; r < 3; ++r) { C[sp6(r, r)] = 2.0 * k_f; C[sp6(3 + r, 3 + r)] = 2.0 * k_m; }
    for (int r = 0; r < 6; ++r) cu[r] = 0.0;
    cu[2] = -2.0 * k_f * mT * DAT_GRAVITY;
    if (v == 1) {
      // Av = [I/mT, Bv], Aw = [0, JTi]: C += 2 (Av'Av + Aw'Aw)
      const double im = S.inv_mT;
      for (int r = 0; r < 3; ++r) {
        C[sp6(r, r)] += 2.0 * im * im;
        for (int c = 0; c < 3; ++c) C[sp6(r, 3 + c)] += 2.0 * im * S.Bv[3 * r + c];
      }
      for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c) {
          double s = 0.0;
          for (int k = 0; k < 3; ++k) s += S.Bv[3 * k + r] * S.Bv[3 * k + c] + JTi[3 * k + r] * JTi[3 * k + c];
          C[sp6(3 + r, 3 + c)] += 2.0 * s;
        }
      double ev[3] = {bv[0] - acc[0], bv[1] - acc[1], bv[2] - acc[2]};
      double ew[3] = {bw[0] - acc[3], bw[1] - acc[4], bw[2] - acc[5]};
      double t[3], s3[3];
      mtv3(S.Bv, ev, t);
      mtv3(JTi, ew, s3);
      for (int r = 0; r < 3; ++r) {
        cu[r] += 2.0 * im * ev[r];
        cu[3 + r] += 2.0 * (t[r] + s3[r]);
      }
    }
  }
  if (with_K) {
    for (int k = 0; k < 22; ++k) S.K[k] = 0.0;
    const double I3[6] = {1, 0, 0, 1, 0, 1};
    for (int j = 0; j < n; ++j) {
      double Rt[9];
      make_Rt(prm + DAT_P_RCOM(n) + 3 * j, Rl, Rt);
      add_UDUt(S.K, Rt, I3, 1.0);
    }
  }

  // base rows (control/rqp_cadmm.py:406-430).  Tilt: (Rl hat(wl))[2,2] = Rl[2,:].(wl x e3),
  // (Rl hat(wl)^2)[2,2] = Rl[2,:].(wl x (wl x e3)).
  S.bmask = 0;
  S.infeasible = 0;
  double e3[3] = {0, 0, 1}, a[3], b[3];
  cross3(wl, e3, a);
  cross3(wl, a, b);
  double al[NBASE][3] = {{-Rl[7], Rl[6], 0.0},
                         {-2.0 * wl[0], -2.0 * wl[1], -2.0 * wl[2]},
                         {-2.0 * vl[0], -2.0 * vl[1], -2.0 * vl[2]}};
  double beta[NBASE] = {dot3(Rl + 6, b) + 2.0 * dot3(Rl + 6, a) + (Rl[8] - prm[DAT_P_COSP]),
                        prm[DAT_P_MAXWL2] - dot3(wl, wl), prm[DAT_P_MAXVL2] - dot3(vl, vl)};
  for (int l = 0; l < NBASE; ++l) {
    for (int c = 0; c < 3; ++c) S.rows[l][c] = al[l][c];
    if (al[l][0] == 0.0 && al[l][1] == 0.0 && al[l][2] == 0.0) {
      if (beta[l] < 0.0) S.infeasible = 1;  // 0 >= -beta fails: the QP is infeasible
      S.rows[l][3] = 1.0;                   // 0 >= 0 carries no information: padding row
      continue;
    }
    S.rows[l][3] = beta[l] + dot3(al[l], l < NWROW ? bw : bv);
    S.bmask |= 1 << l;
  }
}
__host__ __device__ inline __attribute__((noinline)) void build_shared(QPShared& S, const double* prm, int n,
                                                                        const double* st, const double* acc,
                                                                        double k_f, double k_m, int variants,
                                                                        bool with_K) {
  build_shared_inl(S, prm, n, st, acc, k_f, k_m, variants, with_K);
}

// env rows (dvl): lhs . dvl >= rhs  <=>  lhs . lin_v(u) + (lhs . bv - rhs) >= 0.  Rows the
// reference would emit are compacted to the front of the slots (P.emask = bits 0 .. k-1); a row
// with lhs = 0 carries no information and is dropped (infeasible if its constant is negative).
// Slot writes are predicated on compile-time indices so a register-resident E stays in registers.
template <int NB>
DAT_HD void set_env_rows(QPLane<NB>& P, EnvRows& E, const QPShared& S, unsigned mask, const double lhs[DAT_NENV][3],
                         const double rhs[DAT_NENV]) {
  P.infeasible = 0;
#pragma unroll
  for (int j = 0; j < DAT_NENV; ++j) {
    // inactive slots hold the padding row 0 . x + 1 >= 0
    E.a[j][0] = 0.0; E.a[j][1] = 0.0; E.a[j][2] = 0.0;
    E.b[j] = 1.0;
  }
  int k = 0;
#pragma unroll
  for (int j = 0; j < DAT_NENV; ++j) {
    const bool on = (mask >> j) & 1u;
    // a row whose coefficients vanish against its constant (|lhs| <= 1e-12 |rhs|: a rounding remnant, it would
    // need accelerations beyond 1e12 to bind) is a zero row
    const bool zero = lhs[j][0] * lhs[j][0] + lhs[j][1] * lhs[j][1] + lhs[j][2] * lhs[j][2] <= 1e-24 * rhs[j] * rhs[j];
    if (on && zero && -rhs[j] < 0.0) P.infeasible = 1;
    if (!on || zero) continue;
    const double bj = -rhs[j] + dot3(lhs[j], S.bv);
#pragma unroll
    for (int s = 0; s <= j; ++s) {
      if (s == k) {
        E.a[s][0] = lhs[j][0]; E.a[s][1] = lhs[j][1]; E.a[s][2] = lhs[j][2];
        E.b[s] = bj;
      }
    }
    ++k;
  }
  P.emask = (1u << k) - 1u;
}

// Certified infeasibility of an agent QP's dvl rows (the |vl| base row, slot 2, and the env rows): a . x + b >= 0
// with x = lin_v(u) in R^3.  In the C-ADMM (and DD) agent QP the aggregate w is free, so u is free and the QP is
// infeasible exactly when its row system is (the cone block alone is feasible; the two dwl rows act on another
// coordinate of u).  By Helly's theorem an empty intersection of half-spaces in R^3 has an empty subsystem of at
// most 4 rows, and one of at most 3 when their normals lie in a plane (the env rows of vertical trees are
// horizontal): a Farkas certificate lambda >= 0, sum_m lambda_m a_m = 0, sum_m lambda_m b_m < 0, with lambda the
// signed cofactors of the subsystem -- two antiparallel normals, three coplanar ones (scalar cross products in
// their plane) or four that positively span R^3 (3 x 3 determinants).  Degenerate subsystems are skipped, by the
// same 1e-9 of the normals' scale: a triple with a parallel pair, a 4-set with a coplanar triple (their cofactors
// are rounding remnants, nonzero under fused multiply-adds; what they could certify a smaller subsystem does).
// Only strict certificates count: lambda of
// one sign with every entry above 1e-9 of their sum, and a violation beyond 1e-6 of the rows' scale; anything
// closer is left to the IPM, so a certified QP is one whose residuals the IPM cannot bring into band either, and
// one Clarabel reports infeasible (the reference then holds the previous solution, control/rqp_cadmm.py:496-499).
// At most C(11, 2) + C(11, 3) + C(11, 4) = 550 subsystems: the tail kernel runs it once per scenario and step
// (an infeasible agent QP otherwise runs 2 x 50 IPM iterations in every ADMM pass of a stall).
template <class SH, class ER>
DAT_HD bool dvl_rows_infeasible(const SH& sh, const ER& er, unsigned emask) {
  const int ne = __builtin_popcount(emask);  // active env rows: slots 0 .. ne - 1 (set_env_rows compacts them)
  const bool vrow = (sh.get().bmask >> 2) & 1;
  const int m = ne + (vrow ? 1 : 0);
  auto row = [&](int k, double* a, double& b) {
    if (vrow && k == ne) {
      double r4[4];
      ldn<4>(sh.get().rows[2], r4);
      a[0] = r4[0]; a[1] = r4[1]; a[2] = r4[2];
      b = r4[3];
    } else {
      er.ab(k, a, b);
    }
  };
  auto nrm = [](const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
  // lambda (of one sign, normalised positive) certifies infeasibility
  auto cert = [](int q, const double* lam, const double* bb, const double* na) -> bool {
    double sg = lam[0] < 0.0 ? -1.0 : 1.0, tot = 0.0;
    for (int t = 0; t < q; ++t) tot += fabs(lam[t]);
    double lb = 0.0, sc = 0.0;
    for (int t = 0; t < q; ++t) {
      const double l = sg * lam[t];
      if (!(l > 1e-9 * tot)) return false;
      lb += l * bb[t];
      sc += l * (fabs(bb[t]) + na[t]);
    }
    return lb < -1e-6 * sc;
  };
  bool inf = false;
#pragma unroll 1
  for (int i = 0; i < m - 1; ++i) {
    double a1[3], b1;
    row(i, a1, b1);
    const double n1 = nrm(a1);
#pragma unroll 1
    for (int j = i + 1; j < m; ++j) {
      double a2[3], b2, c12[3];
      row(j, a2, b2);
      const double n2 = nrm(a2);
      cross3(a1, a2, c12);
      const double nc12 = nrm(c12);
      if (nc12 <= 1e-9 * n1 * n2 && dot3(a1, a2) < 0.0) {  // antiparallel pair
        const double lam[2] = {n2, n1}, bb[2] = {b1, b2}, na[2] = {n1, n2};
        inf = inf || cert(2, lam, bb, na);
      }
#pragma unroll 1
      for (int k = j + 1; k < m; ++k) {
        double a3[3], b3, c23[3], c31[3];
        row(k, a3, b3);
        const double n3 = nrm(a3);
        cross3(a2, a3, c23);
        cross3(a3, a1, c31);
        const double l4 = -dot3(c12, a3);  // -det(a1, a2, a3)
        const bool flat = fabs(l4) <= 1e-9 * n1 * n2 * n3;
        // a triple with a (anti)parallel pair has no plane of its own: its cross products are rounding remnants
        // (the pair itself is visited above)
        if (flat && nc12 > 1e-9 * n1 * n2 && nrm(c23) > 1e-9 * n2 * n3 && nrm(c31) > 1e-9 * n3 * n1) {
          // coplanar triple: scalar cross products in the plane
          const double* nv = c12;
          if (nrm(c23) > nrm(nv)) nv = c23;
          if (nrm(c31) > nrm(nv)) nv = c31;
          const double lam[3] = {dot3(nv, c23), dot3(nv, c31), dot3(nv, c12)}, bb[3] = {b1, b2, b3},
                       na[3] = {n1, n2, n3};
          inf = inf || cert(3, lam, bb, na);
        }
#pragma unroll 1
        for (int l = k + 1; l < m; ++l) {
          double a4[3], b4, c34[3];
          row(l, a4, b4);
          cross3(a3, a4, c34);
          const double n4 = nrm(a4);
          const double lam[4] = {dot3(a2, c34), -dot3(a1, c34), dot3(c12, a4), l4}, bb[4] = {b1, b2, b3, b4},
                       na[4] = {n1, n2, n3, n4};
          // a 4-set with a coplanar triple spans no simplex: the certificate, if any, is that triple's (visited
          // above), and when every triple is coplanar (rank <= 2) all four cofactors are rounding remnants of
          // no fixed sign -- the 1e-9 test relative to their own sum would pass them
          const bool simplex = !flat && fabs(lam[0]) > 1e-9 * n2 * n3 * n4 && fabs(lam[1]) > 1e-9 * n1 * n3 * n4 &&
                               fabs(lam[2]) > 1e-9 * n1 * n2 * n4;
          inf = inf || (simplex && cert(4, lam, bb, na));
        }
      }
    }
  }
  return inf;
}

// ------------------------------------------------------------------ per-agent data
template <int NB>
DAT_HD void lane_common(QPLane<NB>& P, const double* prm) {
  P.min_fz = prm[DAT_P_MINFZ];
  P.max_f = prm[DAT_P_MAXF];
  P.sec = prm[DAT_P_SEC];
  P.emask = 0u;
  P.infeasible = 0;
  P.tuned = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) { P.atil[r] = 0.0; P.cw[r] = 0.0; }
  P.rho = 1.0;
  P.a2 = 0.0;
}

// C-ADMM agent i (control/rqp_cadmm.py:26-501): variables f in R^{3 x n} (agent i's full copy).
// Cost: Phi(u) with k = 0.1/n, k_feq ||f_i - f_eq_i||^2, leader terms, <lam, f> + rho/2 ||f||^2
// - <rho fbar, f>  ==  rho/2 ||f - a||^2 + const with a = fbar - lam / rho.
// Only f_i carries cones; f_j (j != i) are free and eliminated through (K, atil).
DAT_HD void lane_cadmm_static(QPLane<1>& P, const double* prm, int i) {
  lane_common(P, prm);
  P.var = (i == 0) ? 1 : 0;
}
// per-iteration part: penalty rho and a = fbar - lam / rho.  lam, fbar: (3n) agent-major;
// Rt_all: n x 9.
DAT_HD void lane_cadmm_dynamic(QPLane<1>& P, const double* prm, int n, int i, const double* Rt_all,
                               const double* lam, const double* fbar, double rho, int rt_stride = 9) {
  const double kfeq = prm[DAT_P_KFEQ];
  const double irho = 1.0 / rho;
  P.rho = rho;
  P.kappa = 2.0 * kfeq + rho;
  const double* feq = prm + DAT_P_FEQ(n) + 3 * i;
#pragma unroll
  for (int r = 0; r < 6; ++r) P.atil[r] = 0.0;
  double a2 = 0.0;
  for (int j = 0; j < n; ++j) {
    double a[3] = {fbar[3 * j] - lam[3 * j] * irho, fbar[3 * j + 1] - lam[3 * j + 1] * irho,
                   fbar[3 * j + 2] - lam[3 * j + 2] * irho};
    if (j == i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) P.q[0][c] = -2.0 * kfeq * feq[c] - rho * a[c];
    } else {
      double t[6];
      U_apply(Rt_all + rt_stride * j, a, t);
#pragma unroll
      for (int r = 0; r < 6; ++r) P.atil[r] += t[r];
      a2 += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    }
  }
  P.a2 = a2;
}
// agent i's copy of agent j != i: f_j = a_j - U_j' pi / rho  (stationarity of the free blocks)
DAT_HD void cadmm_free_block(const double* Rt_j, const double* lam_j, const double* fbar_j, const double* pi,
                             double rho, double* f_j) {
  double t[3];
  Ut_apply(Rt_j, pi, t);
  const double irho = 1.0 / rho;
#pragma unroll
  for (int c = 0; c < 3; ++c) f_j[c] = fbar_j[c] - (lam_j[c] + t[c]) * irho;
}

// DD agent i (control/rqp_dd.py:27-505): variables (f_i, F_i, M_i); with w = (F_i, M_i),
// u = U_i f_i + w.  Cost Phi(u) + k_feq ||f_i - f_eq_i||^2 + c_fi'f_i + (c_Fi, c_Mi)'w.
DAT_HD void lane_dd_static(QPLane<1>& P, const double* prm, int i) {
  lane_common(P, prm);
  P.var = (i == 0) ? 1 : 0;
  P.kappa = 2.0 * prm[DAT_P_KFEQ];
}
// prices c = (c_fi, c_Fi, c_Mi) (control/rqp_dd.py:718-722)
DAT_HD void set_dd_price(QPLane<1>& P, const double* prm, int n, int i, const double* c9) {
  const double* feq = prm + DAT_P_FEQ(n) + 3 * i;
  const double kfeq = prm[DAT_P_KFEQ];
#pragma unroll
  for (int c = 0; c < 3; ++c) P.q[0][c] = -2.0 * kfeq * feq[c] + c9[c];
#pragma unroll
  for (int r = 0; r < 6; ++r) P.cw[r] = c9[3 + r];
}

// Centralized (control/rqp_centralized.py:27-448): all n agents' forces, k = 0.1, leader terms on.
// Rt (NB x 9) receives the U-maps of every block.
template <int NB>
DAT_HD void lane_cent(QPLane<NB>& P, const double* prm, int n, const double* st, double Rt[NB][9]) {
  lane_common(P, prm);
  P.var = 1;
  const double kfeq = prm[DAT_P_KFEQ];
  const double* Rl = st + DAT_S_RL(n);
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    const double* feq = prm + DAT_P_FEQ(n) + 3 * k;
    make_Rt(prm + DAT_P_RCOM(n) + 3 * k, Rl, Rt[k]);
#pragma unroll
    for (int c = 0; c < 3; ++c) P.q[k][c] = -2.0 * kfeq * feq[c];
  }
  P.kappa = 2.0 * kfeq;
}


}  // namespace dat

// the interior-point solver of the reduced QP (ipm_solve, ipm_solve_rows)
#include "dat_ipm.hpp"
