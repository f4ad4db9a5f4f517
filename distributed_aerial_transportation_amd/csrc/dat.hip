// dat.hip -- gfx950 kernels and the C-ABI (include/dat.h) of the batched agent-QP solver.
//
// Kernels (all fp64, no MFMA -- every contraction is <= 6 wide):
//   k_cadmm    C-ADMM control step: one 64-lane wavefront holds floor(64/n) scenarios x n agents,
//              one lane per agent QP; the whole ADMM loop (reference control/rqp_cadmm.py:631-675)
//              runs on chip: agent QPs (ipm_solve), consensus mean / residual through LDS, dual
//              update; per-scenario convergence masks.
//   k_dd_setup DD quasi-Newton matrix H = A Q^-1 A' and its inverse per scenario, in LDS
//              (control/rqp_dd.py:513-555, 634-657).
//   k_dd       DD control step: prices, agent QPs, consensus error, dual ascent through H^-1
//              (control/rqp_dd.py:659-752).
//   k_cent     centralized QP, one lane group per scenario and one lane per agent's force
//              (control/rqp_centralized.py:436-448): dat_cent.hip.
//   k_rollout_agents  low-level SO(3) law + dynamics + Lie integration, one lane per agent.
//   k_desired  forest desired-acceleration law (example/rqp_example.py:33-59).
//   k_pmrl_rollout, k_pmrl_forward  point-mass rigid-link system (system/point_mass_rigid_link.py:135-254), one
//              lane per link, the link tensions from a 6 x 6 system replicated on the scenario's lanes
//              (dat_pmrl_step.hpp).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include <algorithm>
#include <chrono>

#include "../../include/dat.h"
#include "dat_ckpt.hpp"
#include "dat_kargs.hpp"
#include "dat_dd_step.hpp"
#include "dat_pmrl_step.hpp"

using namespace dat;

#ifdef DAT_CAPTURE_LOOSE
// development builds only (tools/capture_loose.py): the inputs of the tail's agent QPs accepted in band beyond
// Clarabel's 1e-8 -- [0] scenario, [1] agent, [2] ADMM pass, [3] rho, [4] previous step's passes, [5] forest,
// [6] merit, [7] fused step, [8, 14) acc_des, then the state (S), the agent's multipliers (3n) and the mean (3n)
namespace dat {
constexpr int CAP_MAX = 64, CAP_DOUBLES = 320;
__device__ double g_cap[CAP_MAX][CAP_DOUBLES];
__device__ unsigned int g_ncap;
}  // namespace dat
#endif

namespace {

thread_local std::string g_err;

int fail(const std::string& m) {
  g_err = m;
  return -1;
}

#define HIPCHK(x)                                                                 \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// ------------------------------------------------------------------------------------------------
// C-ADMM
// ------------------------------------------------------------------------------------------------
// A control step runs as three launches:
//   k_env_class   one lane per agent: env CBF rows of the step (they depend on the state only, so
//                 they are fixed for the whole ADMM loop, control/rqp_cadmm.py:305), per-scenario
//                 env class (the largest env-row count among its agents' QPs: 0, <= 2, <= 5,
//                 <= 10), collision, min env distance, and a sort key (class, previous step's
//                 ADMM iteration count); the rows go to HBM (erows / emask, SoA over agents) and
//                 k_cadmm loads them when a slot takes the scenario instead of re-running the query;
//   k_bucket      counting sort of the scenario ids by key (one queue per class; the order within a
//                 key is not fixed, see k_bucket);
//   k_cadmm       persistent blocks (CUs x 4) drain the class queues, classes 3, 2, 1, 0 in turn,
//                 each with its own row-slot instantiation of the IPM (3 + {10, 5, 2, 0} slots:
//                 the register footprint follows the rows the class needs); a scenario slot that
//                 stops is refilled from the queue (cadmm_drain).
// Each scenario's arithmetic does not depend on the scenarios it shares a wavefront with (padding
// rows add exact zeros), so the regrouping does not change any result.
//
// LDS layout of one 64-lane block (G = floor(64/n) scenarios).  Per-lane records use an odd
// stride in doubles so that the 32 lanes of a ds_read_b64 group fall on distinct bank pairs.
//   fbar G x 3n    consensus mean
//   Rt   G x 9n    hat(r_com_j) Rl'
//   sh   G x QPShared (u-maps, packed Hessians, base rows, K)            done / sid / wmx: G ints each
//   area, laid out per env class:
//     rows  the IPM's row state (RowLds: s, z, zw of NR slots x 64 lanes, 3 NR x 64 doubles); the
//           consensus exchange slots red (64 x RDS) alias it: they are used only between solves
//     env   EnvLdsN image of the class's env slots (structure of arrays over the 64 lanes)
// The row state goes to LDS for classes 1 and 2 when their image fits the 40 KB a wavefront may
// hold at four wavefronts per CU (cadmm_rows_lds); class 0 (3 slots) and class 3 (13 slots) keep it
// in registers.  n = 6: class 0 34.8 KB (rows + aux slots), 1 27.3 KB, 2 37.8 KB, 3 39.3 KB (C4 A/B,
// k_cadmm ms: rows of classes 0-2 in LDS 5.53, classes 1-2 5.45, class 2 only 5.51).  Round 4 trimmed
// the exchange slots (RDS 9 -> 7) and the per-slot ints (3 x 64 -> 3 G): class 3's carve was 41.9 KB,
// which with the 256 B of static LDS left room for three workgroups per CU (one SIMD idle); four fit after
// the trim (C4 A/B 3.83 / 3.80 -> 3.72 / 3.77 ms per step), and the budget then went to classes 1 and 2's
// aux groups at three per CU instead (LDS_WAVE_BUDGET).
// (The DD warm start -- k_dd's agent QPs start from the previous pass's iterate from pass DD_WARM_PASS on -- is a
// rule of the DD step: dat_dd_step.hpp states it and what it measured; k_dd has no cold build any more.)
constexpr int RDS = 7;  // consensus exchange slots per lane: mean (3) or F / M totals (6), total residual at [6]
// LDS budget of one k_cadmm workgroup: 53 KB = three per CU.  Four per CU (40 KB) bought ~2 % (§5 of
// DESIGN.md, round 4); the 13 KB more per workgroup hold classes 1 and 2's IPM aux groups in LDS
// instead (C4 A/B 3.79 / 3.80 -> 3.75 / 3.74 ms per step).
constexpr size_t LDS_WAVE_BUDGET = 53 * 1024;
__host__ __device__ constexpr int cadmm_nr(int cls) { return NBASE + class_env_rows(cls); }
// G: scenario slots per wavefront (cadmm_slots)
// doubles rounded up to a 16-byte multiple: every LDS region starts 16-byte aligned (pair reads)
__host__ __device__ constexpr size_t al2(size_t d) { return (d + 1) & ~(size_t)1; }
// per-slot ints done / sid / wmx (G each), rounded to 16 bytes
__host__ __device__ constexpr int slot_ints(int G) { return (3 * G + 3) & ~3; }
__host__ __device__ inline size_t cadmm_fixed_bytes(int n, int G) {
  return sizeof(double) * (al2((size_t)G * 3 * n) + (size_t)G * RT_STRIDE * n) + sizeof(QPShared) * (size_t)G +
         sizeof(int) * (size_t)slot_ints(G);
}
// IPM per-iteration quantities moved to LDS aux slots (ipm_solve AUXM) per env class, when the class's
// carve still fits the budget: class 0 all groups (its 3 row slots leave room; class-0 probe scratch
// traffic 145 -> 23 ops per IPM pass; A/B on MI355X: C2 12.1 -> 11.0 ms, C5 80.7 -> 73.2 ms per step);
// classes 1 and 2 all groups since round 4, at three workgroups per CU (LDS_WAVE_BUDGET; class 3's 13
// row slots do not fit).
// C-ADMM consensus mean and residual read agent-major, the three components of a block together
// (bitwise equal to the component-major loops; C4 A/B: k_cadmm 3.68 / 3.63 -> 3.57 / 3.54 ms)
__host__ __device__ constexpr unsigned cadmm_auxm(int cls) { return cls < NCLS - 1 ? 15u : 0u; }
// row-state placement of a class: 0 registers, 1 LDS rows, 2 LDS rows + the class's aux slots, 3 LDS rows + all
// aux slots (k_cadmm_tail: one scenario per wavefront, latency-bound, every class in LDS)
constexpr unsigned TAIL_AUXM = 15u;
__host__ __device__ constexpr int cadmm_aux_doubles(int cls, int rmode) {
  return rmode == 2 ? ipm_aux_doubles(1, cadmm_auxm(cls)) : rmode == 3 ? ipm_aux_doubles(1, TAIL_AUXM) : 0;
}
__host__ __device__ inline size_t cadmm_area_doubles(int cls, int rmode) {
  const size_t rows = rmode ? (size_t)row_lds_doubles(cadmm_nr(cls), cadmm_aux_doubles(cls, rmode)) : 0;
  return (rows > 64 * RDS ? rows : 64 * RDS) + (size_t)env_lds_doubles(class_env_rows(cls));
}
// row state of class cls in LDS: with the class's aux slots when that carve fits the budget, else rows
// alone for classes ROWLDS_MIN_CLS .. 2; class 3 (13 slots) never.  Few row slots without aux slots
// are cheaper in registers: an LDS row access costs an LDS round trip, which pays only once the rows
// would otherwise spill.
constexpr int ROWLDS_MIN_CLS = 1;
__host__ __device__ inline int cadmm_row_mode(int n, int G, int cls) {
  if (cls >= NCLS - 1) return 0;
  if (cadmm_auxm(cls) && cadmm_fixed_bytes(n, G) + sizeof(double) * cadmm_area_doubles(cls, 2) <= LDS_WAVE_BUDGET)
    return 2;
  if (cls >= ROWLDS_MIN_CLS && cadmm_fixed_bytes(n, G) + sizeof(double) * cadmm_area_doubles(cls, 1) <= LDS_WAVE_BUDGET)
    return 1;
  return 0;
}
// dynamic LDS of a k_cadmm workgroup: the largest carve of the env classes that can occur (without a
// forest every scenario is class 0, so the launch needs only that carve and more workgroups fit a CU)
__host__ __device__ inline size_t cadmm_lds_bytes(int n, int G, int max_cls = NCLS - 1) {
  size_t m = 0;
  for (int c = 0; c <= max_cls; ++c) {
    const size_t b = cadmm_fixed_bytes(n, G) + sizeof(double) * cadmm_area_doubles(c, cadmm_row_mode(n, G, c));
    m = b > m ? b : m;
  }
  return m;
}
// dynamic LDS of a k_cadmm_tail workgroup (one scenario slot, rmode 3), with the n lanes' IPM scratch records
// (best iterate, stiff-row columns and Schur factor: best_size(1) doubles each) behind the class's area: the
// robust solver's stiff-row loops read and write them at every iteration, an LDS round trip instead of L2 / HBM
// k_cadmm_tail: bit-identical clones per agent lane (the lanes a one-scenario wavefront leaves idle), one per
// stiff-row column of the robust solver at most
__host__ __device__ inline int tail_clones(int n) {
  const int v = 64 / (n > 0 ? n : 1);
  return v < 1 ? 1 : v < IPM_NSTIFF ? v : IPM_NSTIFF;
}
__host__ __device__ inline size_t cadmm_tail_lds_bytes(int n, int max_cls = NCLS - 1) {
  size_t m = 0;
  for (int c = 0; c <= max_cls; ++c) {
    const size_t b = cadmm_fixed_bytes(n, 1) + sizeof(double) * (cadmm_area_doubles(c, 3) + al2((size_t)n * best_size(1)));
    m = b > m ? b : m;
  }
  return m;
}
struct CadmmLds {
  double *fbar, *Rt, *red, *rows;
  QPShared* sh;
  double* env;
  int* done;  // per slot: the scenario stopped in this pass
  int* sid;   // per slot: scenario id, -1 empty, -2 retired (queue drained)
  int* wmx;   // per slot: IPM iterations of the scenario's slowest agent QP so far this step
};
__device__ inline CadmmLds cadmm_carve(double* smem, int n, int G, int cls, int rmode) {
  CadmmLds L;
  L.fbar = smem;
  L.Rt = L.fbar + al2(G * 3 * n);
  L.sh = (QPShared*)(L.Rt + G * RT_STRIDE * n);
  L.done = (int*)(L.sh + G);
  L.sid = L.done + G;
  L.wmx = L.sid + G;
  L.rows = (double*)(L.done + slot_ints(G));
  L.red = L.rows;
  const int ra = rmode ? row_lds_doubles(cadmm_nr(cls), cadmm_aux_doubles(cls, rmode)) : 0;
  L.env = L.rows + (ra > 64 * RDS ? ra : 64 * RDS);
  return L;
}

// order-preserving unsigned key of a double (negative values included) for the running minimum of the env
// distance (atomicMin on the key): the sign bit flipped for x >= 0, every bit for x < 0
__host__ __device__ inline unsigned long long dist_key(double x) {
  unsigned long long b;
  memcpy(&b, &x, sizeof(b));
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__host__ __device__ inline double dist_of_key(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  double x;
  memcpy(&x, &b, sizeof(x));
  return x;
}

// env class of one agent QP: 0 if it carries no env row, otherwise the smallest class whose slots
// hold the rows set_env_rows keeps (nonzero rows, compacted).  An all-zero row with a positive
// right-hand side (0 >= rhs > 0: the reference's QP is infeasible, set_env_rows flags it) also
// needs an env class.
__device__ inline int env_class_of(unsigned emask, const double lhs[DAT_NENV][3], const double rhs[DAT_NENV]) {
  bool need = false;
  int k = 0;
#pragma unroll
  for (int j = 0; j < DAT_NENV; ++j) {
    const bool on = (emask >> j) & 1u;
    const bool zero = lhs[j][0] == 0.0 && lhs[j][1] == 0.0 && lhs[j][2] == 0.0;
    need = need || (on && (!zero || rhs[j] > 0.0));
    k += (on && !zero) ? 1 : 0;
  }
  if (!need) return 0;
  int c = 1;
  while (c < NCLS - 1 && k > class_env_rows(c)) ++c;
  return c;
}

// Env rows of the n agents of each scenario of a 64-lane block, computed cooperatively
// (control/rqp_cadmm.py:307-373 from env_rows' pieces, dat_core.hpp).  The payload capsule and the x-window of
// candidate trees are the same for every agent of a scenario; only the camera-cone filter differs
// (cos 100 deg: most agents see most trees).  Lane i of a scenario evaluates trees base + i of each
// chunk of n candidates -- range test, capsule_tree distance and the CBF row, once per tree instead
// of once per agent that sees it -- and publishes them in LDS; then every lane runs its own cone
// filter and sorted insertion over the chunk in tree order.  The pieces and the insertion order are env_rows',
// so the rows are bitwise identical by construction (test_gpu_env_rows_reference.py checks it).
// Must be called by every lane of the block (barriers inside).
constexpr int ENV_CE = 8;  // published entry: in range, c.x, c.y, dd, l3[3], r1
// LDS stride of a published entry: 9 doubles (18 dwords), so the 32 lanes of a ds_*_b64 half-wave
// start on 32 distinct even banks (a stride of 8 doubles put 64 lanes on 4 bank pairs: 16-way conflicts)
constexpr int ENV_CS = ENV_CE + 1;
__device__ EnvOut env_rows_coop(const double* prm, int n, const double* st, const double* trees, int ntree, int i,
                                int ls, bool valid, double alpha_env, unsigned* mask, double lhs[DAT_NENV][3],
                                double rhs[DAT_NENV], double* ent /* LDS: 64 x ENV_CS */) {
  EnvOut out;
  out.collision = 0;
  out.min_env_dist = valid ? prm[DAT_P_VISR] : 0.0;
  *mask = 0u;
  const bool any = valid && trees != nullptr && ntree > 0;
  bool dead = !any;  // this agent keeps no row (it still evaluates its share of the trees)
  EnvFrame fr;
  EnvCam cam;
  int t0 = 0;
  if (any) {
    env_frame(prm, n, st, fr);
    if (!env_camera(prm, n, st, i, cam)) {
      out.collision = 1;
      dead = true;
    }
    t0 = env_window_begin(fr, trees, ntree);
  }
  EnvSeen seen;
  env_clear(seen, lhs, rhs);
  double* mine = ent + (size_t)threadIdx.x * ENV_CS;
  const double* grp = ent + (size_t)(ls * n) * ENV_CS;
  for (int base = t0;; base += n) {
    // this lane's tree of the chunk
    const int t = base + i;
    const bool cand = any && t < ntree && trees[3 * t] <= fr.ctr[0] + fr.reach;
    double e[ENV_CE] = {0, 0, 0, 1e300, 0, 0, 0, 0};
    if (cand) {
      const double* c = trees + 3 * t;
      if (env_in_range(fr, c)) {
        e[0] = 1.0; e[1] = c[0]; e[2] = c[1];
        e[3] = env_tree_row(fr, alpha_env, c, e + 4);
      }
    }
    // every lane of the block takes part in the barriers; the loop ends when no lane had a candidate
    if (!__syncthreads_or(cand)) break;
#pragma unroll
    for (int k = 0; k < ENV_CE; ++k) mine[k] = e[k];
    __syncthreads();
    if (!dead) {
      for (int j = 0; j < n; ++j) {  // the chunk in tree order
        const double* q = grp + (size_t)j * ENV_CS;
        if (q[0] == 0.0) continue;
        if (!env_in_cone(cam, q[1], q[2])) continue;
        const double dd = q[3];
        if (dd < ENV_TOUCH) out.collision = 1;
        env_see(seen, dd, q + 4, lhs, rhs);
      }
    }
    __syncthreads();  // the chunk is consumed before the next one is published
  }
  if (!dead && seen.cnt > 0 && fr.speed > 0.0) {
    out.min_env_dist = seen.dmin;
    *mask = env_mask(seen);
  }
  return out;
}

// The body of k_env_class for the lanes of one block (lane ls * n + i: agent i of scenario sc; valid: the scenario
// takes part), stated once for k_env_class and k_advance.  Every lane of the block must call it (barriers inside).
// nd, cl, md: 64 words of LDS each; ent: 64 x ENV_CS doubles.  lhs, rhs: the lane's sorted row slots, the
// kernel's own arrays: declared here they would be optimised once with this function and again with the kernel
// it is inlined into, and come out wholly scalarised, past the register bound (k_env_class: 180 B/lane of scratch
// against 88 before the body was factored out; as the kernel's, none at 230 VGPRs).
template <int ADV>
__device__ __forceinline__ void env_class_lanes(const KArgs& a, int n, int lane, int ls, int i, int sc, bool valid,
                                                int* nd, int* cl, double* md, double* ent, double lhs[DAT_NENV][3],
                                                double rhs[DAT_NENV]) {
  int need = 0, col = 0;
  double dist = 1e300;
  const double* prm = valid ? prm_of(a, sc) : a.params;
  const double* trees = nullptr;
  int nt = 0;
  if (valid) forest_of(a, sc, &trees, &nt);
  unsigned emask;
  EnvOut e = env_rows_coop(prm, n, valid ? a.state + (size_t)sc * a.S : nullptr, trees, nt, i, ls, valid,
                           prm[DAT_P_AENVD], &emask, lhs, rhs, ent);
  if (valid) {
    need = env_class_of(emask, lhs, rhs);
    col = e.collision;
    dist = e.min_env_dist;
    // hand the rows to k_cadmm (lanes hold consecutive agents: every store is coalesced)
    const size_t NA = (size_t)a.B * n, g = (size_t)sc * n + i;
    a.emask[g] = emask;
#pragma unroll
    for (int j = 0; j < DAT_NENV; ++j) {
      if (!((emask >> j) & 1u)) continue;  // only the slots the mask marks are read back
      a.erows[(4 * j + 0) * NA + g] = lhs[j][0];
      a.erows[(4 * j + 1) * NA + g] = lhs[j][1];
      a.erows[(4 * j + 2) * NA + g] = lhs[j][2];
      a.erows[(4 * j + 3) * NA + g] = rhs[j];
    }
  }
  nd[lane] = need;
  cl[lane] = col;
  md[lane] = dist;
  __syncthreads();
  int cnum = 0;
  double cmin = 1e300;
  if (valid && i == 0) {
    int cls = 0, c = 0;
    double m = prm_of(a, sc)[DAT_P_VISR];
    for (int k = 0; k < n; ++k) {
      cls = max(cls, nd[ls * n + k]);
      c |= cl[ls * n + k];
      m = fmin(m, md[ls * n + k]);
    }
    // previous step's ADMM iterations, then its slowest agent QP's IPM iterations: within a class the
    // longest scenarios are claimed first and scenarios sharing a wavefront tend to need similar
    // numbers of ADMM passes and of IPM iterations per pass (a pass lasts as long as its slowest lane)
    // (beside the running drain the two come as the drain published them: write-through, read past the caches)
    const int pit = ADV == ADV_EARLY ? ld_wt(a.iters + sc) : a.iters[sc];
    const int pmx = ADV == ADV_EARLY ? ld_wt(a.ipmx + sc) : a.ipmx[sc];
    const int bin = NPB * iter_bin(pit) + ipm_bin(pmx);
    // a scenario wedged in a stall (previous step > TAIL_PREV passes) goes to the tail (key NKEY + class); with
    // sub-batches it stays in k_cadmm's queue, which hands it over after its first pass (the tail rule), the
    // same arithmetic
    a.need[sc] = a.route && tail_wedged(pit, a.tail_prev) ? NKEY + cls : cls * NIB + (NIB - 1 - bin);
    a.col[sc] = (unsigned char)c;
    a.mind[sc] = m;
    cnum = c;
    cmin = m;
  }
  // collisions and the smallest env distance of the step (bench stats; one atomic per wavefront, the minimum only
  // when it undercuts the running one)
  for (int off = 32; off > 0; off >>= 1) {
    cnum += __shfl_xor(cnum, off);
    cmin = fmin(cmin, __shfl_xor(cmin, off));
  }
  if (lane == 0) {
    if (cnum) atomicAdd(a.counters + CNT_COLL, (unsigned long long)cnum);
    // (an order-preserving key of the signed distance: a collided payload's distance is negative)
    unsigned long long* pm = a.counters + CNT_COLL + 1;
    const unsigned long long key = dist_key(cmin);
    if (cmin == cmin && key < *(volatile unsigned long long*)pm) atomicMin(pm, key);
  }
}
// Two wavefronts per SIMD (256 VGPRs at most): the build without the bound (290 registers, no scratch, one wavefront
// per SIMD) measured slower, C4 A/B 3.58 / 3.61 -> 3.70 / 3.80 ms per step (round 4).  Three or four wavefronts
// per SIMD (168 / 128 VGPRs, the sorted row slots spilled) measured 3.2-3.6x slower by kernel trace: 0.24 ->
// 0.77 / 0.87 ms (round 4).
// ADV (dat_kargs.hpp): the scenarios that take part; a scenario's lanes do together or not at all, the others are
// carried through the barriers like the lanes past the batch.  ADV_ALL compiles to the kernel without a gate.
template <int ADV>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_env_class(KArgs a) {
  __shared__ int nd[64], cl[64];
  __shared__ double md[64];
  __shared__ double ent[64 * ENV_CS];
  const int n = a.n, G = 64 / n, NT = G * n;
  const int lane = threadIdx.x;
  const int ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  const bool valid = (lane < NT) && (sc < a.B) && adv_gate<ADV, false>(a, sc);
  if constexpr (ADV != ADV_ALL)
    if (!__syncthreads_or(valid)) return;  // no scenario of the block takes part
  double lhs[DAT_NENV][3], rhs[DAT_NENV];
  env_class_lanes<ADV>(a, n, lane, ls, i, sc, valid, nd, cl, md, ent, lhs, rhs);
}

// Counting sort of the scenario ids by key (need[] in [0, NKEY)): list holds the ids of key 0, then
// key 1, ...; count is the class table (ScountRow, dat_kargs.hpp): size / start of env class c (keys c NIB ..
// c NIB + NIB - 1), its queue heads zeroed.  Within a class the key is the previous step's (ADMM
// iterations, slowest agent's IPM iterations) bin, in decreasing order, so the longest scenarios are
// claimed first.  One BUCKET_T-thread workgroup, coalesced strided reads, LDS atomics for the
// histogram and the scatter cursors: the order within a key is not fixed, which only changes which
// scenarios share a wavefront, never a scenario's arithmetic (the capped-grid test compares two
// different groupings bitwise).
constexpr int BUCKET_T = 1024;
static_assert(NKEY_ALL <= BUCKET_T, "bucket_sort initialises one key per thread");
// ADV_EARLY / ADV_REST: ... of the scenarios whose early-rollout mark adv[] is / is not `serial`: the step
// pipeline's two drains of a step take disjoint lists.  A tail-routed scenario (key >= NKEY) goes to the ADV_REST
// list wherever it was advanced, so that a step's routed scenarios run in one tail launch: the tail launches of the
// two drains share a stream, and two of them holding stalled scenarios run one after the other.  need[] of a
// scenario the early pass left out may be stale (its env rows are not computed yet) and is not read by the ADV_EARLY
// sort.  ADV_ALL: every scenario (adv is not read).
// Does the sort of mode ADV list scenario q?
template <int ADV>
__device__ __forceinline__ bool sort_takes(int q, const int* need, const int* adv, int serial) {
  if constexpr (ADV == ADV_ALL) return true;
  else return (adv[q] == serial && need[q] < NKEY) == (ADV == ADV_EARLY);
}
// The class table of a sorted list from its keys' sizes and starts (one thread)
__device__ __forceinline__ void class_table(int* count, const int* tot, const int* kstart) {
  int st = 0;
  for (int cl = 0; cl < NCLS; ++cl) {
    int sz = 0;
    for (int b = 0; b < NIB; ++b) sz += tot[cl * NIB + b];
    count[sc_at(SC_SIZE, cl)] = sz;
    count[sc_at(SC_START, cl)] = st;
    count[sc_at(SC_HEAD, cl)] = 0;       // queue head of the class (k_cadmm)
    count[sc_at(SC_HAND_SIZE, cl)] = 0;  // hand-over list of the class (k_cadmm -> k_cadmm_tail) and its head
    count[sc_at(SC_HAND_HEAD, cl)] = 0;
    st += sz;
  }
  for (int cl = 0; cl < NCLS; ++cl) {  // the tail-routed stretches (keys NKEY + class) behind them
    count[sc_at(SC_TAIL_SIZE, cl)] = tot[NKEY + cl];
    count[sc_at(SC_TAIL_START, cl)] = kstart[NKEY + cl];
    count[sc_at(SC_TAIL_HEAD, cl)] = 0;
  }
}
__device__ __forceinline__ int sort_key(int need) { return min(max(need, 0), NKEY_ALL - 1); }
template <int ADV>
__device__ __forceinline__ void bucket_sort(int B, const int* need, int* list, int* count, const int* adv,
                                            int serial) {
  const auto take = [&](int q) { return sort_takes<ADV>(q, need, adv, serial); };
  __shared__ int hist[NKEY_ALL], kstart[NKEY_ALL], cursor[NKEY_ALL], tot[NKEY_ALL];
  const int t = threadIdx.x;
  if (t < NKEY_ALL) { hist[t] = 0; cursor[t] = 0; }
  __syncthreads();
  for (int q = t; q < B; q += BUCKET_T)
    if (take(q)) atomicAdd(&hist[sort_key(need[q])], 1);
  __syncthreads();
  if (t == 0) {
    int st = 0;
    for (int k = 0; k < NKEY_ALL; ++k) { kstart[k] = st; tot[k] = hist[k]; st += hist[k]; }
  }
  __syncthreads();
  for (int q = t; q < B; q += BUCKET_T) {
    if (!take(q)) continue;
    const int key = sort_key(need[q]);
    list[kstart[key] + atomicAdd(&cursor[key], 1)] = q;
  }
  if (t == 0) class_table(count, tot, kstart);
}
__global__ __launch_bounds__(BUCKET_T) void k_bucket(int B, const int* need, int* list, int* count) {
  bucket_sort<ADV_ALL>(B, need, list, count, nullptr, 0);
}
template <int ADV>
__global__ __launch_bounds__(BUCKET_T) void k_bucket_adv(int B, const int* need, int* list, int* count,
                                                         const int* adv, int serial) {
  static_assert(ADV == ADV_EARLY || ADV == ADV_REST, "the unfiltered sort is k_bucket");
  bucket_sort<ADV>(B, need, list, count, adv, serial);
}

// The filtered sort behind k_advance, which has counted the keys where it made them: a key table (KeyTab) holds the
// histogram of exactly the scenarios sort_takes<ADV> lists -- the early k_advance counts a scenario with a key below
// NKEY into the main drain's table and a tail-routed one into the rest drain's, the late one everything into the
// rest drain's -- so the sort is the scatter alone, over SCATTER_T scenarios per block.  Every block derives the key
// starts from the counts (first wavefront, three keys per lane); a block ranks its scenarios within their keys in
// LDS and claims a stretch per key it holds with one cursor atomic (the order within a key is not fixed, as in
// bucket_sort); block 0 writes the class table.  (A claim per wavefront and key, one after the other, left the
// 65,536-scenario sort at the single workgroup's 66 us: 1,024 wavefronts' claims queue on the few keys most
// scenarios share.)
// The tables alternate (two per drain kind): the last block zeroes `other`, the table of the same kind whose
// previous reader ended before this kernel started and whose next k_advance starts after it has ended
// (closed_loop_pipelined), so no launch waits for a zeroed table.
constexpr int SCATTER_T = 256;
constexpr int KT_COUNT = 0, KT_CURSOR = NKEY_ALL, KT_INTS = 2 * NKEY_ALL;  // KeyTab: counts, then scatter cursors
static_assert(NKEY_ALL <= 3 * 64, "k_bucket_scatter scans three keys per lane of one wavefront");
static_assert(NKEY_ALL <= SCATTER_T, "k_bucket_scatter claims one key per thread");
template <int ADV>
__global__ __launch_bounds__(SCATTER_T) void k_bucket_scatter(int B, const int* need, int* list, int* count,
                                                              const int* adv, int serial, int* tab, int* other) {
  static_assert(ADV == ADV_EARLY || ADV == ADV_REST, "the unfiltered sort is k_bucket");
  __shared__ int kstart[NKEY_ALL], tot[NKEY_ALL], hist[NKEY_ALL], base[NKEY_ALL];
  const int t = threadIdx.x;
  if (t < NKEY_ALL) hist[t] = 0;
  if (t < 64) {  // exclusive prefix sum of the counts
    int c[3], s = 0;
    for (int j = 0; j < 3; ++j) {
      const int k = 3 * t + j;
      c[j] = k < NKEY_ALL ? tab[KT_COUNT + k] : 0;
      s += c[j];
    }
    int incl = s;
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off);
      if (t >= off) incl += v;
    }
    int st = incl - s;
    for (int j = 0; j < 3; ++j) {
      const int k = 3 * t + j;
      if (k < NKEY_ALL) { kstart[k] = st; tot[k] = c[j]; }
      st += c[j];
    }
  }
  __syncthreads();
  const int q = blockIdx.x * SCATTER_T + t;
  const bool take = q < B && sort_takes<ADV>(q, need, adv, serial);
  const int key = take ? sort_key(need[q]) : -1;
  // the block's rank within its key (LDS), then one claim per key the block holds, all keys' claims in flight together
  const int rank = take ? atomicAdd(&hist[key], 1) : 0;
  __syncthreads();
  if (t < NKEY_ALL && hist[t]) base[t] = atomicAdd(tab + KT_CURSOR + t, hist[t]);
  __syncthreads();
  const int pos = take ? kstart[key] + base[key] + rank : -1;
  if ((unsigned)pos < (unsigned)B) list[pos] = q;  // (within the list whatever the tables hold)
  if (blockIdx.x == 0 && t == 0) class_table(count, tot, kstart);
  if (blockIdx.x == gridDim.x - 1)
    for (int k = t; k < KT_INTS; k += SCATTER_T) other[k] = 0;
}

// Work counters of one wavefront, flushed once per class it drained.
struct WaveCounters {
  long long qp = 0, ipm = 0, rowit = 0;  // lane-level: agent-QP solves, IPM iterations, x active rows
  long long inband = 0, loose = 0;      // lane-level: solves accepted through the best in-band iterate
  long long refs = 0, corrs = 0;        // lane-level: IPM refinement passes, corrections applied
  long long slot = 0, pass = 0;         // wave-level: sum of (max lane IPM iterations) per pass, passes
  long long cert = 0, stall = 0, warm = 0;  // k_cadmm_tail, lane-level: certified infeasible, stall exits, warm starts
};
// wave-uniform sum (every lane of the wavefront must execute it)
__device__ inline unsigned long long wave_sum(long long v) {
  unsigned long long s = (unsigned long long)v;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}
// The lane-level solve counters of a wavefront (C-ADMM drain, k_dd), one atomic each: agent-QP solves, IPM
// iterations and x active rows to cc[0 .. 2] (the class's counters), in-band accepts and refinement work to
// CNT_INBAND / CNT_REF.  Every lane of the wavefront must execute it.
__device__ __forceinline__ void flush_solve_counters(const KArgs& a, unsigned long long* cc, const WaveCounters& wc) {
  const unsigned long long q = wave_sum(wc.qp), ip = wave_sum(wc.ipm), rw = wave_sum(wc.rowit);
  const unsigned long long ib = wave_sum(wc.inband), lo = wave_sum(wc.loose);
  const unsigned long long rf = wave_sum(wc.refs), co = wave_sum(wc.corrs);
  if (threadIdx.x == 0) {
    atomicAdd(cc, q);
    atomicAdd(cc + 1, ip);
    atomicAdd(cc + 2, rw);
    if (ib) atomicAdd(a.counters + CNT_INBAND, ib);
    if (lo) atomicAdd(a.counters + CNT_INBAND + 1, lo);
    atomicAdd(a.counters + CNT_REF, rf);
    atomicAdd(a.counters + CNT_REF + 1, co);
  }
}

// A persistent 64-lane block drains the queue of env class CLS (the class's stretch of the sorted
// scenario list, claimed one scenario at a time through the class's queue head).  The block holds G scenario
// slots of n lanes; a slot whose scenario stops is refilled with the next scenario of the queue at
// the start of the next ADMM pass, so a wavefront no longer idles until its slowest scenario of a
// fixed group stops (SIMD occupancy: dat_get_class_occupancy).  A scenario's arithmetic does not
// depend on which slot or wavefront runs it.
// Every agent QP is solved as ipm_solve IPM_FAST_REDO defines it: the fast solver, redone by the robust one
// when it does not end cleanly (ipm_unclean).  RB = false (k_cadmm) carries only the fast solver (IPM_FAST): a
// scenario one of whose agent QPs does not end cleanly leaves at the end of that pass's solves with a resume
// record (rres) and goes to its class's hand-over list; so does a scenario whose next pass falls under the tail
// rule (tail_rule, dat_cadmm_step.hpp), at the end of the pass before it.  RB = true (k_cadmm_tail: one
// scenario slot per wavefront) drains the hand-over lists after k_cadmm (tmode 0), resuming each scenario in
// the pass it left (re-solving there only the agent QPs handed over), or the scenarios k_env_class routed to the
// tail before the step, concurrently with k_cadmm (tmode 1), and finishes their steps (and later fused steps).
// The tail's solves: IPM_FAST_REDO with the certificate of infeasible rows (dvl_rows_infeasible, once per
// scenario-step) and, in the passes the tail rule names, the warm start from the agent QP's converged iterate of
// the previous pass and the stall exit (ipm_solve WS).  Built with -ffp-contract=on (multiply-adds fused within
// an expression only), the inlined fast solver computes the same bits in either kernel, and the tail rule
// depends on the scenario's own history: a scenario's results do not depend on which kernel ran which pass.
// ADV: the drain of the closed loop's advance overlap (dat_closed_loop): a stopped scenario's f_des, iters and
// ipmx are stored write-through and stamped in KArgs::done, and k_cadmm's class-0 drain tells the host when its
// queue has been claimed empty.  Without it k_cadmm / k_cadmm0 are compiled without any of that; the tail kernels
// exist once and go by KArgs::done at run time (a second instantiation changes how their solver is inlined).
template <int CLS, bool RB, bool ADV>
__device__ __forceinline__ void cadmm_drain(const KArgs& a) {
  constexpr bool ENV = CLS > 0;
  constexpr int NR = cadmm_nr(CLS);
  constexpr int NE = class_env_rows(CLS);
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int n = a.n, N3 = 3 * n;
  const int G = a.G;  // G <= 64 / n scenario slots (cadmm_slots); the tail: G = 1
  // the tail: V bit-identical clones of each agent lane (clone vi = lane / n) run the agent QP's solve in lockstep
  // and share out its stiff-row columns (ipm_attempt); only clone 0 writes the scenario's outputs
  const int V = RB ? tail_clones(n) : 1;
  const int NT = (RB ? V : G) * n;
  const int lane = threadIdx.x;
  const int vi = RB ? lane / n : 0;
  const int ls = RB ? 0 : lane / n, i = lane - (RB ? vi : ls) * n;
  const int al = RB ? i : lane;  // the lane's column in the row / env / aux images (a clone's: its agent's)
  const int lsc = ls < G ? ls : 0;
  const bool TM = RB && a.tmode == 1;  // the tail-routed stretch of slist (k_env_class), not the hand-over list
  const int first = a.scount[sc_at(TM ? SC_TAIL_START : SC_START, CLS)];
  const int cnt = a.scount[sc_at(TM ? SC_TAIL_SIZE : RB ? SC_HAND_SIZE : SC_SIZE, CLS)];
  if (cnt == 0) {
    // (an empty class 0 is claimed empty from the start: the advance overlap's signal, see the refill)
    if constexpr (ADV && !RB && CLS == 0)
      if (blockIdx.x == 0 && lane == 0)
        __hip_atomic_store(a.qempty, a.serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  int* const qh = a.scount + sc_at(TM ? SC_TAIL_HEAD : RB ? SC_HAND_HEAD : SC_HEAD, CLS);
  const int* const ql = (RB && !TM ? a.rlist : a.slist) + first;
  const int rmode = RB ? 3 : cadmm_row_mode(n, G, CLS);  // wave-uniform
  CadmmLds L = cadmm_carve(smem, n, G, CLS, rmode);
  double* fb = L.fbar + lsc * N3;
  double* rts = L.Rt + lsc * RT_STRIDE * n;
  double* myred = L.red + lane * RDS;
  QPShared& S = L.sh[lsc];
  const LdsRef<QPShared> shr{L.sh, lsc};
  const EnvLdsN<NE> err{L.env, al};
  const RtLds rtr{L.Rt, (lsc * n + i) * RT_STRIDE};
  if (lane < G) L.sid[lane] = -1;
  __syncthreads();

  // per-lane state of the slot's current scenario
  DAT_PHASE_INIT(9);
  QPLane<1> P;
  int sc = -1;  // scenario of this lane's slot (-1: empty)
  const double* prm = nullptr;
  double* lam = nullptr;
  double* cfs = nullptr;  // the scenario's n agent copies f^(j), in the warm-state array (HBM / L2)
  double* myf = nullptr;
  double* bst = nullptr;
  double* wrl = nullptr;  // k_cadmm_tail: the lane's warm-start record
  int iter = 0, prev_iter = 0, qstat = ST_OPTIMAL;
  int kstep = 0;  // fused control steps (dat_control_steps): the slot scenario's current step
  int rmask = -1;  // k_cadmm_tail: the lanes that solve in the current pass (a resumed pass: those handed over)
  double rho = a.rho0;
  WaveCounters wc;
  for (;;) {
    // ---- refill empty slots from the queue
    DAT_PHASE(11);
    if (lane < NT && i == 0 && vi == 0 && L.sid[ls] == -1) {
      const int q = atomicAdd(qh, 1);
      const int s2 = q < cnt ? ql[q] : -2;  // -2: queue drained, slot retires
      // the advance overlap: the first claim past the end of k_cadmm's last queue tells the host that most of the
      // batch is finished and the launch is ramping down (one system-scope store to mapped host memory)
      if constexpr (ADV && !RB && CLS == 0)
        if (q == cnt) __hip_atomic_store(a.qempty, a.serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      L.sid[ls] = s2;
      L.done[ls] = 0;
      L.wmx[ls] = RB && !TM && s2 >= 0 ? a.rres[(size_t)s2 * RRES_INTS + RRES_WMX] : 0;
    }
    __syncthreads();
    const int slot_sc = lane < NT ? L.sid[ls] : -2;
    const bool fresh = slot_sc >= 0 && slot_sc != sc;
    if (fresh) {
      sc = slot_sc;
      prm = prm_of(a, sc);
      const double* st = a.state + (size_t)sc * a.S;
      if (vi == 0) make_Rt(prm + DAT_P_RCOM(n) + 3 * i, st + DAT_S_RL(n), rts + RT_STRIDE * i);
      lam = a.clam + ((size_t)sc * n + i) * N3;
      cfs = a.cf + (size_t)sc * n * N3;
      myf = cfs + i * N3;
      if (vi == 0)
        for (int c = 0; c < 3; ++c) fb[3 * i + c] = a.cfbar[(size_t)sc * N3 + 3 * i + c];
      // (the tail: the lane's record in LDS, behind the env image -- a generic pointer, flat loads go to LDS)
      bst = RB ? L.env + env_lds_doubles(NE) + i * best_size(1) : a.best + ((size_t)sc * n + i) * BEST_REC;
      iter = 0;
      prev_iter = a.iters[sc];  // the previous step's ADMM iterations (rewritten when the scenario stops)
      qstat = ST_OPTIMAL;
      rho = a.rho0;
      kstep = 0;
      rmask = -1;
      if (RB) {
        wrl = a.wrec + ((size_t)sc * n + i) * WREC_SIZE;
        wrl[0] = 0.0;  // no recorded iterate yet
      }
      if (RB && !TM) {
        // where k_cadmm left the scenario (its warm state -- multipliers, copies, the mean -- is in place)
        const int* const rr = a.rres + (size_t)sc * RRES_INTS;
        kstep = rr[RRES_KSTEP];
        iter = rr[RRES_PASS];
        rmask = rr[RRES_LANES];
        for (int q = 0; q < iter; ++q) rho = fmin(rho * a.tau, a.rho_max);  // the pass's rho, as k_cadmm had it
        qstat = a.qstatus[(size_t)sc * n + i];  // the pass's status of a lane not solved again
      }
      if (i == 0 && vi == 0)
        build_shared(S, prm, n, st, a.acc + ((size_t)kstep * a.B + sc) * 6, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, true);
    }
    if (!__syncthreads_or(slot_sc >= 0)) break;  // every slot retired
    DAT_PHASE(12);
    if (fresh) {
      lane_cadmm_static(P, prm, i);
      if (ENV) {
        // the rows k_env_class computed from the same state this step
        const size_t NA = (size_t)a.B * n, g = (size_t)sc * n + i;
        const unsigned emask = a.emask[g];
        double lhs[DAT_NENV][3], rhs[DAT_NENV];
#pragma unroll
        for (int j = 0; j < DAT_NENV; ++j) {
          const bool on = (emask >> j) & 1u;  // unmarked slots are never written (set_env_rows skips them)
          lhs[j][0] = on ? a.erows[(4 * j + 0) * NA + g] : 0.0;
          lhs[j][1] = on ? a.erows[(4 * j + 1) * NA + g] : 0.0;
          lhs[j][2] = on ? a.erows[(4 * j + 2) * NA + g] : 0.0;
          rhs[j] = on ? a.erows[(4 * j + 3) * NA + g] : 0.0;
        }
        EnvRows E;
        set_env_rows(P, E, S, emask, lhs, rhs);
        env_to_lds<NE>(L.env, al, E);  // (clones: the same values to the same column)
        // the tail certifies infeasible rows once per scenario-step (such an agent QP would run 2 x 50 IPM
        // iterations in every pass and end INACCURATE: the previous solution is held either way)
        if (RB && cadmm_certify_rows(P, shr, err)) wc.cert += vi == 0;
      }
    }
    // ---- one ADMM pass of every occupied slot
    DAT_PHASE(14);
    bool active = slot_sc >= 0;
    int it_lane = 0;
    bool hand = false;  // k_cadmm: this lane's solve was not clean (ipm_unclean)
    // k_cadmm with sub-batches (no tail routing, KArgs::route): a wedged scenario leaves before its first pass, and
    // the tail runs its step from there, as it runs a routed one
    const bool wedged = !RB && iter == 0 && tail_wedged(prev_iter, a.tail_prev);
    if (active && wedged) hand = true;
    if (active && !wedged && ((rmask >> i) & 1)) {
      lane_cadmm_dynamic(P, prm, n, i, rts, lam, fb, rho, RT_STRIDE);
      DAT_PHASE(15);
      P.tuned = cadmm_tuned_start(iter, prev_iter);
      double y[1][3], w[6];
      IPMOut o;
      DAT_PHASE(10);
      constexpr unsigned AUXM = cadmm_auxm(CLS);
      constexpr int RM = RB ? IPM_FAST_REDO : IPM_FAST;
      using SHT = LdsRef<QPShared>;
      using ERT = EnvLdsN<NE>;
      if constexpr (RB) {
        // the tail rule: warm start and stall exit in pass iter (the record is kept in every pass)
        const bool wson = tail_rule(iter, prev_iter, a.tail_prev, a.tail_pass);
        wc.warm += vi == 0 && wson && wrl[0] == 1.0;
        o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowLds, TAIL_AUXM, NoGrp, RM, true>(
            shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol, RowLds{L.rows, al},
            NoGrp{}, wrl, wson, vi, V);
        wc.stall += vi == 0 && o.why == 7;
#ifdef DAT_CAPTURE_LOOSE
        if (vi == 0 && inband_loose(o)) {
          const unsigned k = atomicAdd(&g_ncap, 1u);
          if (k < (unsigned)CAP_MAX && 14 + a.S + 6 * n <= CAP_DOUBLES) {
            double* c = g_cap[k];
            c[0] = sc; c[1] = i; c[2] = iter; c[3] = rho; c[4] = prev_iter;
            c[5] = a.scen_forest ? a.scen_forest[sc] : -1; c[6] = o.merit; c[7] = kstep;
            for (int q = 0; q < 6; ++q) c[8 + q] = a.acc[((size_t)kstep * a.B + sc) * 6 + q];
            for (int q = 0; q < a.S; ++q) c[14 + q] = a.state[(size_t)sc * a.S + q];
            for (int q = 0; q < N3; ++q) { c[14 + a.S + q] = lam[q]; c[14 + a.S + N3 + q] = fb[q]; }
          }
        }
#endif
      } else if constexpr (CLS < NCLS - 1 && (CLS >= ROWLDS_MIN_CLS || AUXM != 0)) {
        if (AUXM != 0 && rmode == 2)
          o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowLds, AUXM, NoGrp, RM>(
              shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol, RowLds{L.rows, lane});
        else if (CLS >= ROWLDS_MIN_CLS && rmode == 1)
          o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowLds, 0, NoGrp, RM>(
              shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol, RowLds{L.rows, lane});
        else
          o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowRegs, 0, NoGrp, RM>(
              shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol);
      } else {
        o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowRegs, 0, NoGrp, RM>(
            shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol);
      }
      hand = !RB && ipm_unclean(o);
      DAT_PHASE(9);
      // a solve k_cadmm hands over is counted once, by k_cadmm_tail (its IPM_FAST_REDO runs the fast attempt
      // again): its discarded outcome here is neither an agent-QP solve nor an in-band accept
      const int keep = hand || vi > 0 ? 0 : 1;  // (nor do its iterations enter the pass's slot counts; nor a clone's)
      wc.ipm += keep * o.iters;
      wc.inband += keep * o.inband;
#ifdef DAT_ITER_HIST
      atomicAdd(&g_iter_hist[o.iters < 63 ? o.iters : 63], 1ull);
#endif
      wc.loose += keep * inband_loose(o);
      wc.refs += keep * o.refs;
      wc.corrs += keep * o.corrs;
      it_lane = keep * o.iters;
      wc.rowit += (long long)(keep * o.iters) * (__builtin_popcount(S.bmask) + __builtin_popcount(P.emask));
      wc.qp += keep;
      qstat = o.status;
      if (vi == 0) cadmm_take_solve(o, myf, y[0], rts, RT_STRIDE, lam, fb, rho, n, i, prm + DAT_P_FEQ(n));
    }
    DAT_PHASE(13);
    wc.slot += wave_max(it_lane);  // (the tail's passes: counted apart, CNT_TAIL)
    ++wc.pass;
    if (active) atomicMax(&L.wmx[ls], it_lane);
    rmask = -1;
    // the slot's lanes whose solve k_cadmm hands over (a ballot: the block is one wavefront)
    const unsigned long long hb = __ballot(hand);
    const int hmask = lane < NT ? (int)((hb >> (ls * n)) & ((1ull << n) - 1ull)) : 0;
    // k_cadmm hands the slot's scenario to k_cadmm_tail, which resumes it in pass `iter` and solves there the
    // agent QPs of `lanes`: the mean and the lanes' statuses go with it (multipliers and copies are in place), the
    // resume record, the class's hand-over list, and the slot is freed
    auto hand_over = [&](int lanes) __attribute__((always_inline)) {
      for (int c = 0; c < 3; ++c) a.cfbar[(size_t)sc * N3 + 3 * i + c] = fb[3 * i + c];
      a.qstatus[(size_t)sc * n + i] = qstat;
      if (i == 0) {
        int* const rr = a.rres + (size_t)sc * RRES_INTS;
        rr[RRES_KSTEP] = kstep;
        rr[RRES_PASS] = iter;
        rr[RRES_WMX] = L.wmx[ls];
        rr[RRES_LANES] = lanes;
        a.rlist[first + atomicAdd(a.scount + sc_at(SC_HAND_SIZE, CLS), 1)] = sc;
        L.sid[ls] = -1;
      }
    };
    __syncthreads();
    if (!RB && active && hmask) {
      // an agent QP of the pass was not clean: the tail redoes the pass's unclean solves (the mean of the pass's
      // start, the statuses of the pass's other solves)
      hand_over(hmask);
      active = false;
    }
    if (active) {
      ++iter;
      rho = fmin(rho * a.tau, a.rho_max);
      cadmm_mean_block(cfs, n, i, myred);
    }
    __syncthreads();
    if (active && vi == 0) {
      for (int c = 0; c < 3; ++c) fb[3 * i + c] = myred[c];
    }
    __syncthreads();
    if (active) {
      if (a.use_total_res) {
        myred[6] = cadmm_total_res(myf, fb, n);
      } else {
        cadmm_aggregate_res(cfs, myf, rts, RT_STRIDE, n, i, myred);
      }
    }
    __syncthreads();
    if (active && i == 0 && vi == 0) {
      double res = 0.0;
      const double* rg = L.red + (ls * n) * RDS;
      if (a.use_total_res) {
        for (int k = 0; k < n; ++k) res = fmax(res, rg[RDS * k + 6]);
      } else {
        for (int r = 0; r < 3; ++r) {
          double sF = 0.0, sM = 0.0;
          for (int k = 0; k < n; ++k) {
            sF += fabs(rg[RDS * k + r]);
            sM += fabs(rg[RDS * k + 3 + r]);
          }
          res = fmax(res, fmax(sF, sM));
        }
      }
      bool stop = (res < a.res_tol) || (iter > a.max_iter);
      if (!stop && a.record_err && a.err) a.err[(size_t)sc * (a.max_iter + 1) + iter - 1] = res;
      L.done[ls] = stop ? 1 : 0;
    }
    __syncthreads();
    if (active) {
      if (!L.done[ls]) {
        if (vi == 0) cadmm_dual_update(lam, myf, fb, rho, n);
        // the tail rule holds from the next pass on: all lanes solve there (the mean of this pass goes with it)
        if (!RB && tail_rule(iter, prev_iter, a.tail_prev, a.tail_pass)) hand_over(-1);
      } else {
        // the scenario stopped: write its outputs and free the slot
        if (RB && i == 0 && vi == 0) {  // a scenario-step the tail finished (and, routed before the step, apart)
          atomicAdd(a.counters + CNT_ROB, 1ull);
          if (TM && kstep == 0) atomicAdd(a.counters + CNT_TAIL + 2, 1ull);
        }
        // (ADV: what the early rollout and env rows of the scenario read while this kernel still runs -- f_des,
        // iters, ipmx -- goes out write-through; the closed loop does not fuse steps, so this is the scenario's
        // last one)
        const bool wt = RB ? a.done != nullptr : ADV;  // (k_cadmm: fixed at compile time; the tail: per launch)
        if (vi == 0) {
          for (int c = 0; c < 3; ++c) {
            a.cfbar[(size_t)sc * N3 + 3 * i + c] = fb[3 * i + c];
            // f_app = diag copies (:669-671)
            if (wt) st_wt(a.fdes + (size_t)sc * N3 + 3 * i + c, myf[3 * i + c]);
            else a.fdes[(size_t)sc * N3 + 3 * i + c] = myf[3 * i + c];
          }
          a.qstatus[(size_t)sc * n + i] = qstat;
          if (i == 0) {
            if (wt) {
              st_wt(a.iters + sc, iter);
              st_wt(a.ipmx + sc, L.wmx[ls]);
            } else {
              a.iters[sc] = iter;
              a.ipmx[sc] = L.wmx[ls];
            }
          }
        }
        if (wt) {
          // the stamp follows the wavefront's stores (all the scenario's lanes are in this wavefront).  No fence:
          // the bytes above left the L2 with their stores
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (i == 0 && vi == 0) st_wt(a.done + sc, a.serial);
        }
        if (kstep + 1 < a.ksteps) {
          // fused steps: the scenario's next control step in the same slot (warm f, f_mean, lambda kept;
          // rho and the iteration count restart as in a new control call, control/rqp_cadmm.py:631-640)
          ++kstep;
          prev_iter = iter;
          iter = 0;
          qstat = ST_OPTIMAL;
          rho = a.rho0;
          if (RB) wrl[0] = 0.0;
          if (i == 0 && vi == 0) {
            build_shared(S, prm, n, a.state + (size_t)sc * a.S, a.acc + ((size_t)kstep * a.B + sc) * 6,
                         prm[DAT_P_KFD], prm[DAT_P_KMD], 3, true);
            L.wmx[ls] = 0;
          }
        } else if (i == 0) {
          L.sid[ls] = -1;
        }
      }
    }
    __syncthreads();
  }
  // work counters of this class: one atomic per wavefront
  unsigned long long* const cc = a.counters + CNT_STRIDE * CLS;
  flush_solve_counters(a, cc, wc);
  const unsigned long long ce = RB ? wave_sum(wc.cert) : 0, sx = RB ? wave_sum(wc.stall) : 0;
  const unsigned long long wm = RB ? wave_sum(wc.warm) : 0;
  if (lane == 0) {
    if (RB) {  // the tail's occupancy apart from k_cadmm's class counters
      unsigned long long* ct = a.counters + CNT_TAIL;
      atomicAdd(ct, (unsigned long long)wc.pass);
      atomicAdd(ct + 1, (unsigned long long)wc.slot);
      if (ce) atomicAdd(ct + 3, ce);
      if (sx) atomicAdd(ct + 4, sx);
      if (wm) atomicAdd(ct + 5, wm);
    } else {
      atomicAdd(cc + 3, (unsigned long long)(wc.slot * NT));
      atomicAdd(cc + 4, (unsigned long long)(wc.pass * G));
    }
  }
  __syncthreads();
}

// The C-ADMM control step of every scenario: persistent blocks drain the env classes in order of
// decreasing row count (the longest-running scenarios first), each class with its own row-slot
// instantiation of the IPM.  All wavefronts work on the same class at (nearly) the same time: the
// unrolled IPM of one class is ~80-130 KB of code, and wavefronts of different classes sharing a
// CU's instruction cache measured 16 % slower (proportional class starts: 12.9 vs 11.1 ms, C4 path).
template <bool ADV>
__global__ __launch_bounds__(64) void k_cadmm(KArgs a) {
  cadmm_drain<3, false, ADV>(a);
  cadmm_drain<2, false, ADV>(a);
  cadmm_drain<1, false, ADV>(a);
  cadmm_drain<0, false, ADV>(a);
}
// The tail: the scenario-steps k_cadmm handed over (an agent QP not clean, or the tail rule) and, launched
// concurrently with k_cadmm, those k_env_class routed here (wedged in a stall), one scenario per wavefront,
// every class's row state and IPM aux slots in LDS: the robust redo, the certificate of infeasible rows, the warm
// start and stall exit of the tail rule's passes.  A kernel of its own: the robust solver compiled into k_cadmm
// cost the fast path 36-60 % (register allocation, C4 A/B).  Without a listed scenario its blocks return at once.
__global__ __launch_bounds__(64) void k_cadmm_tail(KArgs a) {
  cadmm_drain<3, true, false>(a);
  cadmm_drain<2, true, false>(a);
  cadmm_drain<1, true, false>(a);
  cadmm_drain<0, true, false>(a);
}
// Without a forest every scenario is in env class 0 (k_env_class finds no tree): the class-0 drain in a
// kernel of its own, with a 960 B/lane scratch frame instead of k_cadmm's 1,728 (same arithmetic).  C5
// 84.2 / 84.1 -> 80.3 / 79.9 ms per step, C2 12.7 / 12.9 -> 12.0 / 12.1 (round 4, kernel-trace A/B).
// With a forest one launch per class measured 2x slower on C4 (each class launch drains to its own
// tail): k_cadmm keeps the four drains in one launch there.
template <bool ADV>
__global__ __launch_bounds__(64) void k_cadmm0(KArgs a) { cadmm_drain<0, false, ADV>(a); }
__global__ __launch_bounds__(64) void k_cadmm0_tail(KArgs a) { cadmm_drain<0, true, false>(a); }

// ------------------------------------------------------------------------------------------------
// DD: quasi-Newton matrix inverse per scenario (one 64-lane block per scenario)
// ------------------------------------------------------------------------------------------------
// Q_i (strong_convexity_matrix), the eliminations' per-element steps and the H element: dat_dd_step.hpp
// k_dd_setup keeps the columns of [H | I] in registers for n <= DD_REG_NMAX (dd_setup_h_regs), in LDS
// beyond
constexpr int DD_REG_NMAX = 8;
// doubles of the [H | I] area of k_dd_setup; it first holds the per-agent [Q_i | I] (162 n), their
// pivot columns (9 n) and pivot rows (n ints).  Register path: the Q_i area and two N-double pivot
// column buffers only.
__host__ __device__ inline int dd_setup_hs(int n) {
  const int N = 6 * n;
  if (n <= DD_REG_NMAX) return 171 * n + 1 + 2 * N;  // k_dd_setup<n>
  return 2 * N * N > 171 * n + 1 ? 2 * N * N : 171 * n + 1;
}
// dynamic LDS of a k_dd_setup workgroup: the kernel's regions in order and their end.  The kernel carves its smem;
// the host carves from a null base and reads the launch's bytes, so the layout is stated once.
struct DdSetupLds {
  double *Qi, *Rts, *H, *fac, *end;
  size_t bytes() const { return (size_t)((char*)end - (char*)Qi); }
};
__host__ __device__ inline DdSetupLds dd_setup_carve(double* smem, int n) {
  DdSetupLds L;
  L.Qi = smem;                       // n x 81   sym(Q_i^-1)
  L.Rts = L.Qi + 81 * n;             // n x 9
  L.H = L.Rts + 9 * n;               // N x 2N   [H | I]
  L.fac = L.H + dd_setup_hs(n);      // N
  L.end = L.fac + 6 * n;
  return L;
}

// H = A blkdiag(Q_j^-1) A' (control/rqp_dd.py:642-655) and H^-1 by Gauss-Jordan on [H | I], n = NB,
// with the columns of [H | I] in registers: lane c owns column c and, when 2N > 64, column c + 64 (an
// identity column: N <= 48).  Same per-element arithmetic and order as the LDS path, so the result is
// bitwise equal: H_rc summed over blocks j, then over the support p of row r's block in increasing
// order, of A_rp (Q_j A_c)_p with (Q_j A_c)_p summed over q in increasing order; Gauss-Jordan without
// pivoting (H is SPD), per element hk = h_kc / piv, h_rc -= f_r hk.  The column is kept rotated so
// that step k's pivot row is element 0 (no runtime register index): the owner of column k publishes it
// in LDS (double buffered), every lane updates its columns and rotates them by one.
// The elimination's element steps are the header's (dd_hinv_scale, dd_hinv_eliminate).  The assembly restates
// dd_arow / dd_h_element by the row's three cases: here the row r is a compile-time index and the column's agent
// and component are the lane's, so the header's form (a 9-vector per row, zeros skipped by value) would run the
// sums over runtime zeros and index registers at run time.
template <int NB>
__device__ void dd_setup_h_regs(const KArgs& a, int sc, const double* Qi, const double* Rts, double* fac) {
  constexpr int N = 6 * NB;
  constexpr bool TWO = 2 * N > 64;
  const int lane = threadIdx.x;
  double h[N], g[TWO ? N : 1];
  // ---- assembly of column lane (H columns for lane < N, identity columns e_{lane - N} beyond)
#pragma unroll
  for (int r = 0; r < N; ++r) {
    h[r] = (lane >= N && r == lane - N) ? 1.0 : 0.0;
    if (TWO) g[r] = (r == lane + 64 - N) ? 1.0 : 0.0;
  }
  if (lane < N) {
    const int ag = lane / 6, comp = lane - 6 * ag;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const double* Q = Qi + 81 * j;
      // w = Q_j a_{c,j}: a_{c,j} = e_{3+comp} (j == ag), -e_comp (comp < 3), -Rt_j[comp-3, :] on f_j
      double w[9];
      if (j == ag) {
#pragma unroll
        for (int p = 0; p < 9; ++p) { double t = 0.0; t += Q[9 * p + 3 + comp] * 1.0; w[p] = t; }
      } else if (comp < 3) {
#pragma unroll
        for (int p = 0; p < 9; ++p) { double t = 0.0; t += Q[9 * p + comp] * -1.0; w[p] = t; }
      } else {
        const double* rt = Rts + 9 * j + 3 * (comp - 3);
        const double v0 = -rt[0], v1 = -rt[1], v2 = -rt[2];
#pragma unroll
        for (int p = 0; p < 9; ++p) {
          double t = 0.0;
          t += Q[9 * p] * v0;
          t += Q[9 * p + 1] * v1;
          t += Q[9 * p + 2] * v2;
          w[p] = t;
        }
      }
#pragma unroll
      for (int r = 0; r < N; ++r) {
        const int agr = r / 6, cr = r % 6;
        if (j == agr) {
          h[r] += 1.0 * w[3 + cr];
        } else if (cr < 3) {
          h[r] += -1.0 * w[cr];
        } else {
          const double* rt = Rts + 9 * j + 3 * (cr - 3);
          h[r] += -rt[0] * w[0];
          h[r] += -rt[1] * w[1];
          h[r] += -rt[2] * w[2];
        }
      }
    }
  }
  // ---- Gauss-Jordan, columns rotated (h[i] = [H | I]_{(k + i) mod N, c} at step k)
  for (int k = 0; k < N; ++k) {
    double* f = fac + (k & 1) * N;
    if (lane == k) {
#pragma unroll
      for (int i = 0; i < N; ++i) f[i] = h[i];
    }
    __syncthreads();
    const double piv = f[0];
    {
      const double hk = dd_hinv_scale(h[0], piv);
#pragma unroll
      for (int i = 1; i < N; ++i) dd_hinv_eliminate(h[i], f[i], hk);
#pragma unroll
      for (int i = 0; i < N - 1; ++i) h[i] = h[i + 1];
      h[N - 1] = hk;
    }
    if (TWO) {
      const double hk = dd_hinv_scale(g[0], piv);
#pragma unroll
      for (int i = 1; i < N; ++i) dd_hinv_eliminate(g[i], f[i], hk);
#pragma unroll
      for (int i = 0; i < N - 1; ++i) g[i] = g[i + 1];
      g[N - 1] = hk;
    }
  }
  // ---- H^-1 = the right half: column N + c' of [H | I] is column c' of H^-1 (row-major output)
  double* out = a.dHinv + (size_t)sc * N * N;
  if (lane >= N && lane < 2 * N) {
#pragma unroll
    for (int r = 0; r < N; ++r) out[(size_t)r * N + (lane - N)] = h[r];
  }
  if (TWO && lane + 64 < 2 * N) {
#pragma unroll
    for (int r = 0; r < N; ++r) out[(size_t)r * N + (lane + 64 - N)] = g[r];
  }
}

// NB = n (<= DD_REG_NMAX: H columns in registers, one instantiation per team size so each has its own
// register footprint) or 0 (any n: H in LDS)
template <int NB>
__global__ __launch_bounds__(64) void k_dd_setup(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int n = a.n, N = 6 * n;
  const int sc = blockIdx.x;
  const int lane = threadIdx.x;
  if (sc >= a.B) return;
  const DdSetupLds L = dd_setup_carve(smem, n);
  const double* prm = prm_of(a, sc);
  const double* st = a.state + (size_t)sc * a.S;
  // Q_i^-1 by Gauss-Jordan with partial pivoting (np.linalg.inv) on [Q_i | I] in LDS, spread over
  // the wavefront: lane pairs (agent j, column c) update one column each, with the per-element
  // arithmetic of the serial elimination (pivot column copied before the update).
  double* Aug = L.H;                       // n x 9 x 18, in the [H | I] area (built afterwards)
  double* colk = Aug + 162 * n;            // n x 9: column k before step k's update
  int* pivr = (int*)(colk + 9 * n);        // n
  if (lane < n) {
    double Q[81];
    dd_strong_convexity(prm, n, st, lane, Q);
    dd_qinv_augment(Q, Aug + 162 * lane);
    make_Rt(prm + DAT_P_RCOM(n) + 3 * lane, st + DAT_S_RL(n), L.Rts + 9 * lane);
  }
  __syncthreads();
  for (int k = 0; k < 9; ++k) {
    if (lane < n) pivr[lane] = dd_qinv_pivot_row(Aug + 162 * lane, k);
    __syncthreads();
    for (int e = lane; e < 18 * n; e += 64) {  // row exchange k <-> p, column by column
      const int j = e / 18, c = e - 18 * j;
      dd_qinv_exchange(Aug + 162 * j, k, pivr[j], c);
    }
    __syncthreads();
    for (int e = lane; e < 9 * n; e += 64) {
      const int j = e / 9, r = e - 9 * j;
      colk[e] = Aug[162 * j + 18 * r + k];
    }
    __syncthreads();
    for (int e = lane; e < 18 * n; e += 64) {
      const int j = e / 18, c = e - 18 * j;
      dd_qinv_update_col(Aug + 162 * j, colk + 9 * j, k, c);
    }
    __syncthreads();
  }
  for (int e = lane; e < 81 * n; e += 64) {
    const int j = e / 81, rc = e - 81 * j, r = rc / 9, c = rc - 9 * r;
    L.Qi[e] = dd_qinv_sym(Aug + 162 * j, r, c);
  }
  __syncthreads();
  if constexpr (NB > 0) {
    dd_setup_h_regs<NB>(a, sc, L.Qi, L.Rts, L.H + 171 * n + 1);  // pivot columns past the Q_i elimination area
    return;
  }
  // H = A blkdiag(Q_j^-1) A'  (control/rqp_dd.py:642-655)
  for (int e = lane; e < N * N; e += 64) {
    int r = e / N, c = e % N;
    L.H[2 * N * r + c] = dd_h_element(L.Qi, L.Rts, n, r, c);
    L.H[2 * N * r + N + c] = (r == c) ? 1.0 : 0.0;
  }
  __syncthreads();
  // Gauss-Jordan on [H | I] (H is SPD: no pivoting needed)
  // Each lane owns whole columns of [H | I] (no index division; a row of the tile is contiguous
  // across lanes, so the LDS accesses are conflict-free); per-element operation order as before.
  for (int k = 0; k < N; ++k) {
    double piv = L.H[2 * N * k + k];
    for (int r = lane; r < N; r += 64) L.fac[r] = L.H[2 * N * r + k];
    __syncthreads();
    for (int c = lane; c < 2 * N; c += 64) dd_hinv_update_col(L.H, 2 * N, N, L.fac, piv, k, c);
    __syncthreads();
  }
  double* out = a.dHinv + (size_t)sc * N * N;
  for (int e = lane; e < N * N; e += 64) out[e] = L.H[2 * N * (e / N) + N + (e % N)];
}

// ------------------------------------------------------------------------------------------------
// DD step
// ------------------------------------------------------------------------------------------------
constexpr int DD_ES = 7, DD_RS = 5;
// k_dd per-wavefront area: with a forest the env rows' LDS image; without one nothing (n = 6:
// 27.0 KB, four wavefronts per CU -- the unused 20 KB image used to hold k_dd at three, C3 A/B
// 23.8 -> 22.7 ms).  The 3 base rows' IPM state stays in registers: RowLds measured 26.2 ms, and rows
// (+ aux slots) in LDS without a forest measured no gain on C3 in round 3 (git history).
__host__ __device__ constexpr int dd_area_doubles(bool env) { return env ? ENV_LDS_DOUBLES : 0; }
constexpr int DD_SLOT_INTS = 64;  // ints of each per-slot array of k_dd (G <= 21 used)
// dynamic LDS of a k_dd workgroup of G = floor(64/n) scenario slots (NT = G n lanes): as DdSetupLds
struct DdLds {
  double *X, *lamF, *lamM, *E, *Rts, *red, *envs;
  QPShared* shs;
  int *sid, *done, *wmx, *lng, *end;
  size_t bytes() const { return (size_t)((char*)end - (char*)X); }
};
__host__ __device__ inline DdLds dd_carve(double* smem, int n, bool env) {
  const int N3 = 3 * n, G = 64 / n, NT = G * n;
  DdLds L;
  L.X = smem;                                       // NT x 9   (f_i, F_i, M_i)
  L.lamF = L.X + al2(NT * 9);                       // G x 3n
  L.lamM = L.lamF + al2(G * N3);                    // G x 3n
  L.E = L.lamM + al2(G * N3);                       // NT x ES  consensus error (ES = 7: odd stride, no bank conflicts)
  L.Rts = L.E + al2(NT * DD_ES);                    // G x n x RT_STRIDE
  L.red = L.Rts + G * RT_STRIDE * n;                // 64 x DD_RS
  L.shs = (QPShared*)(L.red + 64 * DD_RS);          // G
  L.envs = (double*)(L.shs + G);                    // EnvLds image (env only)
  L.sid = (int*)(L.envs + dd_area_doubles(env));    // G: scenario of the slot (-1 empty, -2 retired)
  L.done = L.sid + DD_SLOT_INTS;                    // G: the slot's scenario stopped in this pass
  L.wmx = L.done + DD_SLOT_INTS;                    // G: IPM iterations of the slot's slowest agent QP this step
  L.lng = L.wmx + DD_SLOT_INTS;                     // G: the slot's chain is a long one (dd_long_chain)
  L.end = L.lng + DD_SLOT_INTS;
  return L;
}
// k_dd_key: drain-order key of every scenario -- the previous step's (DD iteration count, slowest agent
// QP's IPM iterations), longest first, as k_cadmm's key -- sorted by k_bucket into one queue (class 0).
// (dd_ipm_bin: dat_dd_step.hpp)
__global__ void k_dd_key(KArgs a) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc < a.B) a.need[sc] = NIB - 1 - (NPB * iter_bin(a.iters[sc]) + dd_ipm_bin(a.ipmx[sc]));
}

// DD control step (control/rqp_dd.py:695-752), persistent: each 64-lane block holds G = floor(64/n)
// scenario slots of n lanes (one lane per agent QP) and drains the sorted scenario queue; a slot whose
// scenario stops is refilled at the next dual-ascent pass.  A scenario's arithmetic does not depend
// on the slot or block that runs it.  ENV = false (no forest on the handle): every QP has the three
// base rows only, and the IPM is instantiated for them alone (the register footprint of the 13-slot
// instantiation is not paid).
template <bool ENV>
__global__ __launch_bounds__(64) void k_dd(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int n = a.n, N3 = 3 * n, N6 = 6 * n;
  const int G = 64 / n, NT = G * n;
  const int lane = threadIdx.x;
  const int ls = lane / n, i = lane - ls * n;
  const int lsc = ls < G ? ls : 0;
  const DdLds L = dd_carve(smem, n, ENV);
  QPShared& S = L.shs[lsc];
  double* myX = L.X + lane * 9;
  const double* Xs = L.X + lsc * n * 9;  // the slot's agent records (dat_dd_step.hpp)
  const double* Es = L.E + lsc * n * DD_ES;
  double* lF = L.lamF + lsc * N3;
  double* lM = L.lamM + lsc * N3;
  double* rts = L.Rts + lsc * RT_STRIDE * n;
  const int cnt = a.scount[sc_at(SC_SIZE, 0)], first = a.scount[sc_at(SC_START, 0)];
  const LdsRef<QPShared> shr{L.shs, lsc};
  const EnvLds err{L.envs, lane};
  const RtLds rtr{L.Rts, (lsc * n + i) * RT_STRIDE};
  if (lane < G) L.sid[lane] = -1;
  __syncthreads();

  QPLane<1> P;
  const double* prm = nullptr;
  const double* Rl = nullptr;
  double* bst = nullptr;
  double* wrl = nullptr;  // the agent QP's warm-start record (HBM)
  double prev[9];
  int sc = -1, iter = 0, qstat = ST_OPTIMAL, col = 0;
  int kstep = 0;  // fused control steps (dat_control_steps): the slot scenario's current step
  double mdist = 0.0;
  WaveCounters wc;
  // phase marks (DAT_PHASE_PROF builds, tools/phase_prof.py): 11 refill + fresh slot setup, 14 prices,
  // 10 ipm_solve, 9 result bookkeeping, 13 consensus error, stop test, dual ascent, outputs
  DAT_PHASE_INIT(11);
  for (;;) {
    DAT_PHASE(11);
    // ---- refill empty slots from the queue
    if (lane < NT && i == 0 && L.sid[ls] == -1) {
      const int q = atomicAdd(a.scount + sc_at(SC_HEAD, 0), 1);
      L.sid[ls] = q < cnt ? a.slist[first + q] : -2;
      L.done[ls] = 0;
      L.wmx[ls] = 0;
      L.lng[ls] = 0;
    }
    __syncthreads();
    const int slot_sc = lane < NT ? L.sid[ls] : -2;
    const bool fresh = slot_sc >= 0 && slot_sc != sc;
    if (fresh) {
      sc = slot_sc;
      prm = prm_of(a, sc);
      const double* st = a.state + (size_t)sc * a.S;
      Rl = st + DAT_S_RL(n);
      make_Rt(prm + DAT_P_RCOM(n) + 3 * i, Rl, rts + RT_STRIDE * i);
      for (int c = 0; c < 3; ++c) {
        lF[3 * i + c] = a.dlamF[(size_t)sc * N3 + 3 * i + c];
        lM[3 * i + c] = a.dlamM[(size_t)sc * N3 + 3 * i + c];
      }
      for (int c = 0; c < 9; ++c) prev[c] = a.dprev[((size_t)sc * n + i) * 9 + c];
      for (int c = 0; c < 9; ++c) myX[c] = prev[c];  // the controller's current (f, F, M)
      bst = a.best + ((size_t)sc * n + i) * BEST_REC;
      wrl = a.wrec + ((size_t)sc * n + i) * WREC_SIZE;
      wrl[0] = 0.0;
      iter = 0;
      qstat = ST_OPTIMAL;
      kstep = 0;
      if (i == 0) build_shared(S, prm, n, st, a.acc + (size_t)sc * 6, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, false);
    }
    if (!__syncthreads_or(slot_sc >= 0)) break;  // every slot retired
    if (fresh) {
      lane_dd_static(P, prm, i);
      col = 0;
      mdist = prm[DAT_P_VISR];
      if (ENV) {
        const double* trees;
        int nt;
        unsigned emask;
        forest_of(a, sc, &trees, &nt);
        double lhs[DAT_NENV][3], rhs[DAT_NENV];
        EnvOut env = env_rows(prm, n, a.state + (size_t)sc * a.S, trees, nt, i, prm[DAT_P_AENVD], &emask, lhs, rhs);
        col = env.collision;
        mdist = env.min_env_dist;
        EnvRows Ev;
        set_env_rows(P, Ev, S, emask, lhs, rhs);
        env_to_lds(L.envs, lane, Ev);
      }
    }
    const bool active = slot_sc >= 0;
    const int nr = wave_max(active ? rows_needed(P.emask) : NBASE);
    DAT_PHASE(14);
    if (active) {
      double c9[9];
      dd_prices(prm, n, i, lF, lM, Rl, c9);
      set_dd_price(P, prm, n, i, c9);
      double y[1][3], w[6];
      IPMOut o;
      const double* y0 = prm + DAT_P_FEQ(n) + 3 * i;
      DAT_PHASE(10);
      // a late pass of a long chain: the agent QP differs from the previous pass's only in its prices, so it starts
      // from that pass's last iterate (ipm_solve WS, the tail kernel's warm start); a long chain's QPs are solved
      // tighter (dd_qp_tol, dat_dd_step.hpp)
      const bool lng = L.lng[ls] != 0;
      const bool wson = dd_warm_start(iter, lng);
      const double qtol = dd_qp_tol(lng, a.qp_tol);
      if constexpr (ENV)
        o = ipm_solve_rows<MODE_DD, 1, IPM_FAST, true>(nr, shr, err, rtr, P, y0, y, w, bst, IPM_MAX_ITER, qtol, wrl,
                                                       wson);
      else
        o = ipm_solve<MODE_DD, 1, NBASE, LdsRef<QPShared>, EnvLds, RtLds, RowRegs, 0, NoGrp, IPM_FAST, true>(
            shr, err, rtr, P, y0, y, w, bst, IPM_MAX_ITER, qtol, RowRegs{}, NoGrp{}, wrl, wson);
      DAT_PHASE(9);
      wc.ipm += o.iters;
      wc.inband += o.inband;
      wc.loose += inband_loose(o);
      wc.refs += o.refs;
      wc.corrs += o.corrs;
      atomicMax(&L.wmx[ls], o.iters);
#ifdef DAT_ITER_HIST
      atomicAdd(&g_iter_hist[o.iters < 63 ? o.iters : 63], 1ull);
#endif
      wc.rowit += (long long)o.iters * (__builtin_popcount(S.bmask) + __builtin_popcount(P.emask));
      ++wc.qp;
      qstat = o.status;
      dd_take_solve(o.status, y[0], w, prm, n, i, Xs, prev);
    }
    DAT_PHASE(13);
    __syncthreads();  // agent 0's fallback above reads X before this pass's writes
    if (active) {
      for (int c = 0; c < 9; ++c) myX[c] = prev[c];
    }
    __syncthreads();
    if (active) {
      ++iter;
      dd_consensus_error(Xs, rts, RT_STRIDE, n, i, L.E + lane * DD_ES);
      L.red[lane * DD_RS + 0] = col ? 1.0 : 0.0;
      L.red[lane * DD_RS + 1] = mdist;
    }
    __syncthreads();
    if (active && i == 0) {
      const double res = dd_pass_residual(Es, DD_ES, n);
      const bool stop = dd_stop(res, a.res_tol, iter, a.max_iter);
      if (!stop && a.record_err && a.err) a.err[(size_t)sc * (a.max_iter + 1) + iter - 1] = res;
      L.done[ls] = stop ? 1 : 0;
      if (!stop && dd_long_chain(iter, res)) L.lng[ls] = 1;
    }
    __syncthreads();
    if (active) {
      if (!L.done[ls]) {
        dd_dual_ascent(a.dHinv + (size_t)sc * N6 * N6 + (size_t)(6 * i) * N6, N6, Es, DD_ES, n, lF + 3 * i, lM + 3 * i);
      } else {
        // the scenario stopped: write its outputs and free the slot
        for (int c = 0; c < 3; ++c) {
          a.dlamF[(size_t)sc * N3 + 3 * i + c] = lF[3 * i + c];
          a.dlamM[(size_t)sc * N3 + 3 * i + c] = lM[3 * i + c];
          a.fdes[(size_t)sc * N3 + 3 * i + c] = myX[c];
        }
        for (int c = 0; c < 9; ++c) a.dprev[((size_t)sc * n + i) * 9 + c] = prev[c];
        a.qstatus[(size_t)sc * n + i] = qstat;
        if (i == 0) {
          a.iters[sc] = iter;
          a.ipmx[sc] = L.wmx[ls];
          int coll = 0;
          double md = prm[DAT_P_VISR];
          for (int k = 0; k < n; ++k) {
            coll |= L.red[(ls * n + k) * DD_RS] != 0.0;
            md = fmin(md, L.red[(ls * n + k) * DD_RS + 1]);
          }
          a.col[sc] = (unsigned char)coll;
          a.mind[sc] = md;
        }
        if (kstep + 1 < a.ksteps) {
          // fused steps (no forest): the scenario's next control step in the same slot, from the warm
          // lambda_F, lambda_M and previous solutions it leaves (control/rqp_dd.py:695-700)
          ++kstep;
          iter = 0;
          wrl[0] = 0.0;
          qstat = ST_OPTIMAL;
          if (i == 0) {
            build_shared(S, prm, n, a.state + (size_t)sc * a.S, a.acc + ((size_t)kstep * a.B + sc) * 6,
                         prm[DAT_P_KFD], prm[DAT_P_KMD], 3, false);
            L.wmx[ls] = 0;
            L.lng[ls] = 0;
          }
        } else if (i == 0) {
          L.sid[ls] = -1;
        }
      }
    }
    __syncthreads();
  }
  flush_solve_counters(a, a.counters, wc);
}

// ------------------------------------------------------------------------------------------------
// rollout / desired acceleration / warm start
// ------------------------------------------------------------------------------------------------
// `steps` simulation steps (sim_step, system/rigid_quadrotor_payload.py:129-222) with one lane per (scenario, agent): G = floor(64/n) scenarios
// per 64-lane block.  Lane i runs agent i's low-level law, rotational dynamics and attitude
// integration; the payload's force / moment sums go through LDS and every lane of the scenario
// integrates the payload identically (sums in agent order, the pieces of sim_step, dat_core.hpp: bitwise
// the same trajectory by construction).  Per-lane state is one quadrotor plus the payload (~40 doubles), so nothing
// spills and the kernel runs many wavefronts per SIMD, for any n (k_rollout<0> kept the whole state
// of a large team in scratch).
//
// LOG = true (a log is open, dat_log_begin): the launch is one HL period of dat_closed_loop and also writes the
// period's records (layouts: dat_layout.h DAT_LOG_*).  On entry lane i of a recorded scenario writes its f_des
// and qp_status, lane 0 the rest of the HL record from the entry state (the HL instant's); lane 0 of every
// scenario writes the summary tier.  At a logged step lane i writes the thrust and moment it applies and, after
// the integration (and the polar projection), its R and w; lane 0 the payload and the tracking errors.  A
// scenario's record is contiguous and a lane's stores are runs of 4, 9 + 3 and 20 doubles, like the state
// write-back below.  LOG = false compiles to the kernel without any of it.
constexpr int RO_X = 6;  // per lane in LDS: u = f R e3 (3), hat(r_com) Rl' u (3)
constexpr double REF_X_OFFSET = 1.5;  // x_ref leads the payload by 1.5 m (example/rqp_example.py:36)
// the mountain record m of scenario sc's desired-acceleration law (without a forest: the flat default)
__device__ inline void mountain_of(const KArgs& a, int sc, double* m) {
  const int f = (a.nforest > 0) ? (a.scen_forest ? a.scen_forest[sc] : 0) : -1;
  if (f < 0 || a.mountain == nullptr) {
    m[DAT_M_CX] = 30.0; m[DAT_M_CY] = 0.0; m[DAT_M_RADIUS] = 25.0; m[DAT_M_SPHERE_R] = 1e300; m[DAT_M_DEPTH] = 0.0;
  } else {
    for (int k = 0; k < DAT_MOUNTAIN_SIZE; ++k) m[k] = a.mountain[(size_t)f * DAT_MOUNTAIN_SIZE + k];
  }
}
// ADV (dat_kargs.hpp): the scenarios that take part.  The early pass runs beside the drain on the scenarios whose
// done stamp is this step's and reads their f_des as the drain published it (write-through, past the caches); it
// marks them in adv, and both passes count their scenarios (advcnt).  ADV_ALL compiles to the kernel without a gate.
// The body of k_rollout_agents for the lanes of one block, stated once for k_rollout_agents and k_advance: the gate
// and its count, the steps, the write-back and the adv[] mark.  xs: 64 x RO_X doubles of LDS.  Returns false when no
// scenario of the block takes part (nothing was done: the kernel returns); *took_part: this lane's scenario took part.
template <bool LOG, int ADV>
__device__ __forceinline__ bool rollout_lanes(const KArgs& a, int steps, double dt, const double* fdes,
                                              const std::conditional_t<LOG, LogArgs, NoLog>& lg, double* xs,
                                              bool* took_part) {
  static_assert(!LOG || ADV == ADV_ALL, "the logging rollout is not gated");
  const int n = a.n, G = 64 / n, NT = G * n;
  const int lane = threadIdx.x, ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  bool valid = lane < NT && sc < a.B;
  if constexpr (ADV != ADV_ALL) {
    // (a scenario's lanes follow its first lane's reading of the stamp)
    valid = __shfl((int)(valid && adv_gate<ADV, true>(a, sc)), (ls * n) & 63) != 0 && valid;
    // (the stamp is read before the bytes it covers: the loads below are issued after this branch)
    asm volatile("" ::: "memory");
    const unsigned long long took = __ballot(valid && i == 0);
    if (!took) return false;  // no scenario of the block takes part (one wavefront: uniform)
    if (lane == 0) atomicAdd(a.advcnt + (ADV == ADV_EARLY ? 0 : 1), (unsigned long long)__builtin_popcountll(took));
  }
  const double* prm = valid ? prm_of(a, sc) : a.params;
  double* g = valid ? a.state + (size_t)sc * a.S : nullptr;
  double R[9], W[3], xl[3], vl[3], Rl[9], wl[3], fd[3];
  int cnt = 0;
  if (valid) {
    for (int k = 0; k < 9; ++k) { R[k] = g[DAT_S_R(n) + 9 * i + k]; Rl[k] = g[DAT_S_RL(n) + k]; }
    for (int c = 0; c < 3; ++c) {
      W[c] = g[DAT_S_W(n) + 3 * i + c];
      xl[c] = g[DAT_S_XL(n) + c];
      vl[c] = g[DAT_S_VL(n) + c];
      wl[c] = g[DAT_S_WL(n) + c];
      fd[c] = ADV == ADV_EARLY ? ld_wt(fdes + (size_t)sc * 3 * n + 3 * i + c) : fdes[(size_t)sc * 3 * n + 3 * i + c];
    }
    cnt = a.counter[sc];
  }
  // LOG: what a lane needs again at a logged step waits in LDS (its slot; lane 0 of a scenario: x_ref, v_ref of
  // this HL period), each word read back by the lane that wrote it (no barrier needed), so the step loop carries no
  // per-lane log state of its own; the next logged step of the launch and its record are the same for every lane
  __shared__ int lslot[LOG ? 64 : 1];
  __shared__ double lref[LOG ? 64 / 3 * 6 : 1];
  [[maybe_unused]] int lnext = 0;
  [[maybe_unused]] double* lrec = nullptr;  // slot 0 of the record of that step
  if constexpr (LOG) {
    const long long first = (lg.clock + lg.log_every - 1) / lg.log_every;  // first logged step / log_every
    lnext = (int)(first * lg.log_every - lg.clock);
    lrec = lg.step + (size_t)(first - lg.step_base) * lg.nslot * DAT_LOG_ST_WORDS(n);
    int slot = -1;
    if (valid) {
      const long long hk = lg.clock / lg.hl_every - lg.hl_base;
      if (i == 0 && lg.sum_iters) {
        const size_t o = (size_t)hk * lg.batch + sc;
        lg.sum_iters[o] = a.iters[sc];
        lg.sum_mind[o] = a.mind[sc];
        lg.sum_col[o] = a.col[sc];
      }
      slot = lg.slot[sc];
      if (slot >= 0) {
        double* r = lg.hl + ((size_t)hk * lg.nslot + slot) * DAT_LOG_HL_WORDS(n);
        int* ri = reinterpret_cast<int*>(r + DAT_LOG_HL_INTS(n));
        for (int c = 0; c < 3; ++c) r[3 * i + c] = fd[c];
        ri[2 + i] = a.qstatus[(size_t)sc * n + i];
        if (i == 0) {
          double m[DAT_MOUNTAIN_SIZE], ref[6];  // x_ref, v_ref
          mountain_of(a, sc, m);
          forest_references(xl, m, REF_X_OFFSET, ref, ref + 3);
          r[DAT_LOG_HL_MIND(n)] = a.mind[sc];
          for (int c = 0; c < 6; ++c) r[DAT_LOG_HL_XREF(n) + c] = lref[6 * ls + c] = ref[c];
          ri[0] = a.iters[sc];
          ri[1] = a.col[sc];
        }
      }
    }
    lslot[lane] = slot;
  }
  const double* J = prm + DAT_P_J(n) + 9 * i;
  const double* Ji = prm + DAT_P_JINV(n) + 9 * i;
  double* mine = xs + lane * RO_X;
  const double* grp = xs + ls * n * RO_X;
  for (int s = 0; s < steps; ++s) {
    double dw[3] = {0, 0, 0};
    if (valid) {
      double f, M[3];
      ll_control_agent(R, W, J, fd, &f, M, a.ll_kind);
      if constexpr (LOG) {
        if (s == lnext && lslot[lane] >= 0) {  // 32-byte aligned: two 16-byte stores
          double2* w = reinterpret_cast<double2*>(lrec + (size_t)lslot[lane] * DAT_LOG_ST_WORDS(n) + 4 * i);
          w[0] = make_double2(f, M[0]);
          w[1] = make_double2(M[1], M[2]);
        }
      }
      double um[RO_X];
      quad_accel(R, W, J, Ji, prm + DAT_P_RCOM(n) + 3 * i, Rl, f, M, dw, um);
      for (int c = 0; c < RO_X; ++c) mine[c] = um[c];
    }
    __syncthreads();
    if (valid) {
      double dvc[3] = {0, 0, 0}, mom[3] = {0, 0, 0}, dvl[3], dwl[3];
      for (int k = 0; k < n; ++k)
        for (int c = 0; c < 3; ++c) { dvc[c] += grp[k * RO_X + c]; mom[c] += grp[k * RO_X + 3 + c]; }
      payload_accel(prm, Rl, wl, dvc, mom, dvl, dwl);
      integrate_rot(R, W, dw, dt);
      integrate_lin(xl, vl, dvl, dt);
      integrate_rot(Rl, wl, dwl, dt);
      if (projection_due(&cnt)) {
        polar3(Rl);
        polar3(R);
      }
      if constexpr (LOG) {
        if (s == lnext && lslot[lane] >= 0) {
          double* rec = lrec + (size_t)lslot[lane] * DAT_LOG_ST_WORDS(n);
          double* q = rec + DAT_LOG_ST_STATE(n);
          for (int k = 0; k < 9; ++k) q[DAT_S_R(n) + 9 * i + k] = R[k];
          for (int c = 0; c < 3; ++c) q[DAT_S_W(n) + 3 * i + c] = W[c];
          if (i == 0) {
            const double* ref = lref + 6 * ls;
            double ex[3], ev[3];
            for (int c = 0; c < 3; ++c) {
              q[DAT_S_XL(n) + c] = xl[c];
              q[DAT_S_VL(n) + c] = vl[c];
              q[DAT_S_WL(n) + c] = wl[c];
              ex[c] = ref[c] - xl[c];
              ev[c] = ref[3 + c] - vl[c];
            }
            for (int k = 0; k < 9; ++k) q[DAT_S_RL(n) + k] = Rl[k];
            rec[DAT_LOG_ST_XERR(n)] = sqrt(dot3(ex, ex));
            rec[DAT_LOG_ST_XERR(n) + 1] = sqrt(dot3(ev, ev));
          }
        }
      }
    }
    if constexpr (LOG) {
      if (s == lnext) {
        lnext += lg.log_every;
        lrec += (size_t)lg.nslot * DAT_LOG_ST_WORDS(n);
      }
    }
    __syncthreads();  // the sums are read before the next step overwrites them
  }
  if (valid) {
    for (int k = 0; k < 9; ++k) g[DAT_S_R(n) + 9 * i + k] = R[k];
    for (int c = 0; c < 3; ++c) g[DAT_S_W(n) + 3 * i + c] = W[c];
    if (i == 0) {
      for (int c = 0; c < 3; ++c) {
        g[DAT_S_XL(n) + c] = xl[c];
        g[DAT_S_VL(n) + c] = vl[c];
        g[DAT_S_WL(n) + c] = wl[c];
      }
      for (int k = 0; k < 9; ++k) g[DAT_S_RL(n) + k] = Rl[k];
      a.counter[sc] = cnt;
      if constexpr (ADV == ADV_EARLY) a.adv[sc] = a.serial;
    }
  }
  *took_part = valid;
  return true;
}
template <bool LOG, int ADV>
__global__ __launch_bounds__(64) void k_rollout_agents(KArgs a, int steps, double dt, const double* fdes,
                                                       std::conditional_t<LOG, LogArgs, NoLog> lg) {
  __shared__ double xs[64 * RO_X];
  bool took;
  (void)rollout_lanes<LOG, ADV>(a, steps, dt, fdes, lg, xs, &took);
}

// lg: the open log's arguments at this launch (dat_closed_loop), or null: the plain kernel
// adv: the pass of the closed loop's advance overlap (ADV_ALL: every scenario)
void launch_rollout(const KArgs& a, int B, hipStream_t stream, int steps, double dt, const double* fdes,
                    const LogArgs* lg = nullptr, int adv = ADV_ALL) {
  const int G = 64 / a.n;
  const dim3 grid((B + G - 1) / G);
  constexpr auto k_log = k_rollout_agents<true, ADV_ALL>;
  constexpr auto k_all = k_rollout_agents<false, ADV_ALL>;
  constexpr auto k_early = k_rollout_agents<false, ADV_EARLY>;
  constexpr auto k_rest = k_rollout_agents<false, ADV_REST>;
  if (lg)
    hipLaunchKernelGGL(k_log, grid, dim3(64), 0, stream, a, steps, dt, fdes, *lg);
  else
    hipLaunchKernelGGL(adv == ADV_EARLY ? k_early : adv == ADV_REST ? k_rest : k_all, grid, dim3(64), 0, stream, a,
                       steps, dt, fdes, NoLog{});
}

// RQPLowLevelController.control (control/rqp_centralized.py:518-535) at the current states: thrust
// f (B x n) and moments M (B x n x 3) from f_des, one lane per (scenario, agent)
__global__ void k_low_level(KArgs a, const double* fdes, double* fo, double* Mo) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = a.n;
  if (t >= a.B * n) return;
  const int sc = t / n, i = t - sc * n;
  const double* prm = prm_of(a, sc);
  const double* st = a.state + (size_t)sc * a.S;
  // (inlined here as in the rollout instantiations: with three callers the inliner would leave a call)
  [[clang::always_inline]] ll_control_agent(st + DAT_S_R(n) + 9 * i, st + DAT_S_W(n) + 3 * i, prm + DAT_P_J(n) + 9 * i,
                                            fdes + (size_t)sc * 3 * n + 3 * i, fo + t, Mo + 3 * (size_t)t, a.ll_kind);
}

// rigid payload (system/rigid_payload.py:93-130): `steps` steps of dt with the forces f held, one lane per scenario
__global__ void k_rp_rollout(KArgs a, int steps, double dt, const double* f) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= a.B) return;
  const int n = a.n;
  const double* prm = prm_of(a, sc);
  double* st = a.state + (size_t)sc * a.S;
  int cnt = a.counter[sc];
  for (int s = 0; s < steps; ++s) rp_step(prm, n, st, &cnt, f + (size_t)sc * 3 * n, dt);
  a.counter[sc] = cnt;
}

// Point-mass rigid-link system (PMRLDynamics, system/point_mass_rigid_link.py:135-254; the pieces of
// dat_pmrl_step.hpp), k_rollout_agents' mapping: one lane per link, G = floor(64/n) scenarios per 64-lane block, idle
// lanes masked.  A lane holds its link (q, dq) and a copy of the payload in registers across the steps.  Per step one
// LDS exchange between one pair of barriers: lane i publishes (m_i, y_i, g_i); every lane of the scenario assembles
// S and G y from the records in link order (identical bits in all of them), solves the 6 x 6 system and integrates
// its own link and its copy of the payload.  Lane 0 of a scenario writes the payload and the counter back.
constexpr int PM_X = 8;  // per lane in LDS: m, y, g (6)
// the accelerations at the lane's state: the lane's T and ddq, the scenario's dvl and dwl (all lanes of a block
// call it, valid or not: it holds the step's two barriers)
__device__ __forceinline__ void pmrl_lane_forward(const double* prm, int n, int i, bool valid, double* mine,
                                                  const double* grp, const double* Rl, const double* wl,
                                                  const double* q, const double* dq, const double* f, double* T,
                                                  double* ddq, double* dvl, double* dwl) {
  PmrlPayload p;
  PmrlLink lk;
  if (valid) {
    pmrl_payload_terms(prm, Rl, wl, p);
    pmrl_link_terms(prm, n, i, p, Rl, q, dq, f, lk);
    mine[0] = prm[DAT_P_PM_M(n) + i];
    mine[1] = lk.y;
    for (int c = 0; c < 6; ++c) mine[2 + c] = lk.g[c];
  }
  __syncthreads();
  if (valid) {
    double S[21], z[6];
    pmrl_system_clear(S, z);
    for (int k = 0; k < n; ++k) {
      double rec[PM_X];
      for (int c = 0; c < PM_X; ++c) rec[c] = grp[k * PM_X + c];
      pmrl_system_add(S, z, rec[0], rec[1], rec + 2);
    }
    pmrl_solve6(S, z);
    PmrlSums s;
    pmrl_payload_accel(prm, n, p, z, s, dvl, dwl);
    *T = pmrl_tension(prm[DAT_P_PM_M(n) + i], lk.y, lk.g, z);
    pmrl_link_accel(prm, n, i, Rl, lk, q, *T, s, ddq);
  }
  __syncthreads();  // the records are read before the next step overwrites them
}
// `steps` steps of dt under the force schedule f[nf][B][3n] (agent-major): step s uses set s / (steps / nf)
__global__ __launch_bounds__(64) void k_pmrl_rollout(KArgs a, int steps, int nf, double dt, const double* f) {
  __shared__ double xs[64 * PM_X];
  const int n = a.n, G = 64 / n, NT = G * n;
  const int lane = threadIdx.x, ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  const bool valid = lane < NT && sc < a.B;
  const double* prm = valid ? prm_of(a, sc) : a.params;
  double* g = valid ? a.state + (size_t)sc * a.S : nullptr;
  double q[3] = {0, 0, 1}, dq[3] = {0, 0, 0}, xl[3], vl[3], Rl[9], wl[3], fi[3] = {0, 0, 0};
  int cnt = 0;
  if (valid) {
    for (int c = 0; c < 3; ++c) {
      q[c] = g[DAT_S_Q(n) + 3 * i + c];
      dq[c] = g[DAT_S_DQ(n) + 3 * i + c];
      xl[c] = g[DAT_S_XL(n) + c];
      vl[c] = g[DAT_S_VL(n) + c];
      wl[c] = g[DAT_S_WL(n) + c];
    }
    for (int k = 0; k < 9; ++k) Rl[k] = g[DAT_S_RL(n) + k];
    cnt = a.counter[sc];
  }
  const int hold = steps / nf;  // steps a force set is held
  const size_t fset = (size_t)a.B * 3 * n;
  const double* fp = f + (valid ? (size_t)sc * 3 * n + 3 * i : 0);
  for (int s = 0, left = 0; s < steps; ++s, --left) {
    if (left == 0) {
      left = hold;
      if (valid)
        for (int c = 0; c < 3; ++c) fi[c] = fp[c];
      fp += fset;
    }
    double T, ddq[3], dvl[3], dwl[3];
    pmrl_lane_forward(prm, n, i, valid, xs + lane * PM_X, xs + ls * n * PM_X, Rl, wl, q, dq, fi, &T, ddq, dvl, dwl);
    if (valid) {
      pmrl_integrate_link(q, dq, ddq, dt);
      pmrl_integrate_payload(xl, vl, Rl, wl, dvl, dwl, dt, &cnt);
    }
  }
  if (valid) {
    for (int c = 0; c < 3; ++c) {
      g[DAT_S_Q(n) + 3 * i + c] = q[c];
      g[DAT_S_DQ(n) + 3 * i + c] = dq[c];
    }
    if (i == 0) {
      for (int c = 0; c < 3; ++c) {
        g[DAT_S_XL(n) + c] = xl[c];
        g[DAT_S_VL(n) + c] = vl[c];
        g[DAT_S_WL(n) + c] = wl[c];
      }
      for (int k = 0; k < 9; ++k) g[DAT_S_RL(n) + k] = Rl[k];
      a.counter[sc] = cnt;
    }
  }
}
// PMRLDynamics.forward_dynamics (:156-208) at the current states, which it leaves alone: ddq (B x 3n, agent-major),
// dvl, dwl (B x 3), T (B x n) under the thrusts f (B x 3n)
__global__ __launch_bounds__(64) void k_pmrl_forward(KArgs a, const double* f, double* ddq_o, double* dvl_o,
                                                     double* dwl_o, double* T_o) {
  __shared__ double xs[64 * PM_X];
  const int n = a.n, G = 64 / n, NT = G * n;
  const int lane = threadIdx.x, ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  const bool valid = lane < NT && sc < a.B;
  const double* prm = valid ? prm_of(a, sc) : a.params;
  const double* g = valid ? a.state + (size_t)sc * a.S : nullptr;
  double q[3] = {0, 0, 1}, dq[3] = {0, 0, 0}, Rl[9], wl[3], fi[3] = {0, 0, 0};
  if (valid) {
    for (int c = 0; c < 3; ++c) {
      q[c] = g[DAT_S_Q(n) + 3 * i + c];
      dq[c] = g[DAT_S_DQ(n) + 3 * i + c];
      wl[c] = g[DAT_S_WL(n) + c];
      fi[c] = f[(size_t)sc * 3 * n + 3 * i + c];
    }
    for (int k = 0; k < 9; ++k) Rl[k] = g[DAT_S_RL(n) + k];
  }
  double T, ddq[3], dvl[3], dwl[3];
  pmrl_lane_forward(prm, n, i, valid, xs + lane * PM_X, xs + ls * n * PM_X, Rl, wl, q, dq, fi, &T, ddq, dvl, dwl);
  if (valid) {
    for (int c = 0; c < 3; ++c) ddq_o[(size_t)sc * 3 * n + 3 * i + c] = ddq[c];
    T_o[(size_t)sc * n + i] = T;
    if (i == 0)
      for (int c = 0; c < 3; ++c) {
        dvl_o[(size_t)sc * 3 + c] = dvl[c];
        dwl_o[(size_t)sc * 3 + c] = dwl[c];
      }
  }
}

// the desired acceleration of scenario sc from its state in memory (k_desired, k_advance)
__device__ __forceinline__ void desired_of(const KArgs& a, int sc, double* acc) {
  const double* st = a.state + (size_t)sc * a.S;
  double* o = acc + (size_t)sc * 6;
  double m[DAT_MOUNTAIN_SIZE];
  mountain_of(a, sc, m);
  desired_accel_forest(st, a.n, m, REF_X_OFFSET, o);
}
template <int ADV>
__global__ void k_desired(KArgs a, double* acc) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= a.B || !adv_gate<ADV, false>(a, sc)) return;
  desired_of(a, sc, acc);
}

// The advance pass of the closed loop in one launch (dat_set_fused_advance): k_rollout_agents<false, ADV>, k_desired<ADV>
// and k_env_class<ADV> of a block's G scenarios, through the same device functions on the same inputs, so a
// scenario's state, acc, env rows and key are bit for bit those of the three launches.  The three share the mapping
// (lane ls * n + i: agent i) and the gate: the scenarios the rollout takes are the ones it marks (ADV_EARLY) or
// finds unmarked (ADV_REST), which is the gate of the other two.  The block barrier orders the state's write-back
// before its reads: k_desired's by the scenario's first lane, the env rows' by every lane, from memory as in the
// separate kernels.  One grid waits once for the SIMDs the drain's wavefronts free, and the state is not fetched
// from memory again.  Registers: bound as k_env_class (256); the rollout's are dead at the barrier.
template <int ADV>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_advance(KArgs a, int steps, double dt,
                                                                                        const double* fdes,
                                                                                        double* acc, int* kc_lo,
                                                                                        int* kc_hi) {
  static_assert(ADV == ADV_EARLY || ADV == ADV_REST, "the ungated step runs the three kernels");
  __shared__ double xs[64 * RO_X];
  __shared__ int nd[64], cl[64];
  __shared__ double md[64];
  __shared__ double ent[64 * ENV_CS];
  const int n = a.n, G = 64 / n;
  const int lane = threadIdx.x, ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  bool valid;
  if (!rollout_lanes<false, ADV>(a, steps, dt, fdes, NoLog{}, xs, &valid)) return;
  __syncthreads();  // the state is stored before it is read back
  if (valid && i == 0) desired_of(a, sc, acc);
  double lhs[DAT_NENV][3], rhs[DAT_NENV];
  env_class_lanes<ADV>(a, n, lane, ls, i, sc, valid, nd, cl, md, ent, lhs, rhs);
  // the sort's count (k_bucket_scatter), where the keys are made: the block's histogram, then one atomic per key it
  // holds into the key table of the list the scenario goes to (kc_lo: keys below NKEY, kc_hi: the tail-routed ones;
  // null: the sort counts for itself)
  if (kc_lo == nullptr) return;
  __shared__ int hist[NKEY_ALL];
  for (int k = lane; k < NKEY_ALL; k += 64) hist[k] = 0;
  __syncthreads();
  if (valid && i == 0) atomicAdd(&hist[sort_key(a.need[sc])], 1);  // (the key this lane has just stored)
  __syncthreads();
  for (int k = lane; k < NKEY_ALL; k += 64)
    if (const int c = hist[k]) atomicAdd((k < NKEY ? kc_lo : kc_hi) + KT_COUNT + k, c);
}

__global__ void k_warm(KArgs a) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= a.B) return;
  const int n = a.n, N3 = 3 * n;
  const double* prm = prm_of(a, sc);
  const double* feq = prm + DAT_P_FEQ(n);
  if (a.cf) {
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < N3; ++c) {
        a.cf[((size_t)sc * n + i) * N3 + c] = feq[c];
        a.clam[((size_t)sc * n + i) * N3 + c] = 0.0;
      }
    for (int c = 0; c < N3; ++c) a.cfbar[(size_t)sc * N3 + c] = feq[c];
  }
  if (a.dlamF) {
    double s3[3] = {0, 0, 0};
    for (int k = 0; k < n; ++k)
      for (int c = 0; c < 3; ++c) s3[c] += feq[3 * k + c];
    for (int c = 0; c < N3; ++c) { a.dlamF[(size_t)sc * N3 + c] = 0.0; a.dlamM[(size_t)sc * N3 + c] = 0.0; }
    for (int i = 0; i < n; ++i) dd_fallback(prm, n, i, s3, a.dprev + ((size_t)sc * n + i) * 9);
  }
  if (a.pf)
    for (int c = 0; c < N3; ++c) a.pf[(size_t)sc * N3 + c] = feq[c];
  for (int c = 0; c < N3; ++c) a.fdes[(size_t)sc * N3 + c] = feq[c];
  // the previous step's ADMM / DD iteration count and slowest IPM count select the IPM start (C-ADMM
  // warm regime) and the drain order: a reset handle behaves exactly like a freshly created one
  a.iters[sc] = 0;
  if (a.ipmx) a.ipmx[sc] = 0;
}

__global__ void k_env(KArgs a, double* lhs, double* rhs, int* nrow, unsigned char* col, double* md) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = a.n;
  if (t >= a.B * n) return;
  const int sc = t / n, i = t % n;
  const double* prm = prm_of(a, sc);
  const double* st = a.state + (size_t)sc * a.S;
  const double* trees;
  int nt, k = 0;
  unsigned mask;
  forest_of(a, sc, &trees, &nt);
  double L[DAT_NENV][3], R[DAT_NENV];
  bool cent = (a.cf == nullptr && a.dlamF == nullptr);
  EnvOut e = env_rows(prm, n, st, trees, nt, cent ? -1 : i, cent ? prm[DAT_P_AENVC] : prm[DAT_P_AENVD], &mask, L, R);
  double* lo = lhs + (size_t)t * DAT_NENV * 3;
  double* ro = rhs + (size_t)t * DAT_NENV;
  for (int r = 0; r < DAT_NENV; ++r) {
    for (int c = 0; c < 3; ++c) lo[3 * r + c] = 0.0;
    ro[r] = 0.0;
  }
#pragma unroll
  for (int r = 0; r < DAT_NENV; ++r) {
    if (!((mask >> r) & 1u)) continue;
    for (int c = 0; c < 3; ++c) lo[3 * k + c] = L[r][c];
    ro[k] = R[r];
    ++k;
  }
  nrow[t] = k;
  col[t] = (unsigned char)e.collision;
  md[t] = e.min_env_dist;
}

// ------------------------------------------------------------------------------------------------
// raw batched agent QPs: RQPPrimalSolver.solve (control/rqp_cadmm.py:482-501, control/rqp_dd.py:475-505)
// ------------------------------------------------------------------------------------------------
// One lane per item (a scenario's state / parameters / forest, one agent, its own multipliers).
// Not a hot path: the scenario data live in lane registers / scratch (PlainRef), as in k_cent.
struct AgentQPArgs {
  int count;
  const int *scen, *agent;
  const double *acc, *lam, *rho, *fbar, *c9;
  double* x;
  int *status, *iters;
  unsigned char* col;
  double* mind;
  double* best;
  // dat_solve_agent_qp_rows_batch: the caller's compacted env rows instead of the forest query (else null)
  const double *elhs, *erhs;
  const int* nenv;
  unsigned char* cert;  // dvl_rows_infeasible returned true
};

__global__ __launch_bounds__(64) void k_agent_qp(KArgs a, AgentQPArgs q) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = k < q.count;
  const int n = a.n, N3 = 3 * n;
  const bool dd = a.dlamF != nullptr;
  const int sc = valid ? q.scen[k] : 0, i = valid ? q.agent[k] : 0;
  const double* prm = prm_of(a, sc);
  const double* st = a.state + (size_t)sc * a.S;
  QPShared S;
  QPLane<1> P;
  EnvRows E;
  double Rt_all[NMAX * 9];
  int nr = NBASE;
  EnvOut env;
  env.collision = 0;
  env.min_env_dist = 0.0;
  if (valid) {
    for (int j = 0; j < n; ++j) make_Rt(prm + DAT_P_RCOM(n) + 3 * j, st + DAT_S_RL(n), Rt_all + 9 * j);
    build_shared(S, prm, n, st, q.acc + (size_t)k * 6, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, !dd);
    if (dd) {
      lane_dd_static(P, prm, i);
    } else {
      lane_cadmm_static(P, prm, i);
    }
    const double* trees;
    int nt;
    unsigned emask;
    double lhs[DAT_NENV][3], rhs[DAT_NENV];
    if (q.elhs) {
      // the caller's rows, compacted (slots 0 .. nenv - 1); no env query: no collision, distance +inf
      emask =
          env_slots_of_rows(q.elhs + (size_t)k * DAT_NENV * 3, q.erhs + (size_t)k * DAT_NENV, q.nenv[k], lhs, rhs);
      env.min_env_dist = INFINITY;
    } else {
      forest_of(a, sc, &trees, &nt);
      env = env_rows(prm, n, st, trees, nt, i, prm[DAT_P_AENVD], &emask, lhs, rhs);
    }
    set_env_rows(P, E, S, emask, lhs, rhs);
    nr = rows_needed(P.emask);
    if (dd) {
      set_dd_price(P, prm, n, i, q.c9 + (size_t)k * 9);
    } else {
      lane_cadmm_dynamic(P, prm, n, i, Rt_all, q.lam + (size_t)k * N3, q.fbar + (size_t)k * N3, q.rho[k]);
    }
  }
  nr = wave_max(nr);
  if (!valid) return;
  double y[1][3], w[6];
  const PlainRef<QPShared> shr{&S};
  const EnvPlain er{&E};
  const RtPtr rtr{Rt_all + 9 * i};
  double* bst = q.best + (size_t)k * best_size(1);
  // the C-ADMM agent QP as the closed loop solves it: rows certified infeasible are held (k_cadmm_tail)
  const bool cert = !dd && cadmm_certify_rows(P, shr, er);
  IPMOut o = dd ? ipm_solve_rows<MODE_DD, 1>(nr, shr, er, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER,
                                             a.qp_tol)
                : ipm_solve_rows<MODE_CADMM, 1, IPM_FAST_REDO>(nr, shr, er, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst,
                                                IPM_MAX_ITER, a.qp_tol);
  if (dd) {
    double* xo = q.x + (size_t)k * 9;
    for (int c = 0; c < 3; ++c) xo[c] = y[0][c];
    for (int c = 0; c < 6; ++c) xo[3 + c] = w[c];
  } else {
    double* xo = q.x + (size_t)k * N3;
    cadmm_copy_of_solve(xo, y[0], o.pi, Rt_all, 9, q.lam + (size_t)k * N3, q.fbar + (size_t)k * N3, q.rho[k], n, i);
  }
  // in-band accepts (rare: per lane, no wavefront reduction)
  if (o.inband) atomicAdd(a.counters + CNT_INBAND, 1);
  if (inband_loose(o)) atomicAdd(a.counters + CNT_INBAND + 1, 1);
  atomicAdd(a.counters + CNT_REF, (unsigned long long)o.refs);
  atomicAdd(a.counters + CNT_REF + 1, (unsigned long long)o.corrs);
  q.status[k] = o.status;
  q.iters[k] = o.iters;
  q.col[k] = (unsigned char)env.collision;
  q.mind[k] = env.min_env_dist;
  q.cert[k] = (unsigned char)cert;
}

// ------------------------------------------------------------------------------------------------
// checkpoint records (dat_checkpoint_save / dat_checkpoint_load; layout: dat_layout.h DAT_CK_*)
// ------------------------------------------------------------------------------------------------
// The record's segments as kernel arguments, written from the table of dat_ckpt.hpp (ck_args): the handle's fp64
// arrays with their words per scenario and record offsets, and the int arrays behind the ints' words (null: the
// mode has no such array; it reads as 0 and is not written).
struct CkArgs {
  int nf, words, ints_off;
  double* f[CK_MAX_FIELDS];
  int w[CK_MAX_FIELDS], off[CK_MAX_FIELDS];
  int* ints[CK_NINTS + 1];
  int *done, *adv;  // scatter: the closed loop's stamps of the scenarios written (null: the mode has none)
};
template <int U>
struct CkUnit;
template <>
struct CkUnit<1> { using T = double; };
template <>
struct CkUnit<2> { using T = double2; };
// the array and the word in it behind word x of scenario sc's record (null: an int word or padding)
__device__ __forceinline__ double* ck_word(const CkArgs& c, int sc, int x) {
  for (int k = 0; k < c.nf; ++k) {
    const int d = x - c.off[k];
    if ((unsigned)d < (unsigned)c.w[k]) return c.f[k] + (size_t)sc * c.w[k] + d;
  }
  return nullptr;
}
// One wavefront per record; its lanes walk the record's words in units of U words (U = 2, 16-byte accesses, where
// every segment's size and offset is even: every source run and every record is then 16-byte aligned; else U = 1),
// so a wavefront instruction reads and writes runs of up to 1 KiB / 512 B that are contiguous within a segment.
// k_ckpt_gather: record r of `out` from scenario list[r] (null: r).
template <int U>
__global__ __launch_bounds__(256) void k_ckpt_gather(CkArgs c, const int* list, int count, double* out) {
  using T = typename CkUnit<U>::T;
  const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
  const long long r = (long long)blockIdx.x * wpb + (threadIdx.x >> 6);
  if (r < count) {
    const int sc = list ? list[r] : (int)r;
    double* rec = out + (size_t)r * c.words;
    for (int x = lane * U; x < c.words; x += 64 * U) {
      double v[2] = {0.0, 0.0};
      if ((unsigned)(x - c.ints_off) < (unsigned)CK_INT_WORDS) {
        for (int j = 0; j < U; ++j) {
          const int i0 = 2 * (x + j - c.ints_off);
          v[j] = __hiloint2double(c.ints[i0 + 1] ? c.ints[i0 + 1][sc] : 0, c.ints[i0] ? c.ints[i0][sc] : 0);
        }
      } else if (const double* p = ck_word(c, sc, x)) {
        const T t = *(const T*)p;
        memcpy(v, &t, sizeof(T));
      }
      T t;
      memcpy(&t, v, sizeof(T));
      *(T*)(rec + x) = t;
    }
  }
}
// k_ckpt_scatter: record rec[r] - base (null: r - base) of `in` into scenario scen[r] (null: r); the scenarios are
// distinct.  Their stamps are cleared: 0 is no step's stamp (next_serial).
template <int U>
__global__ __launch_bounds__(256) void k_ckpt_scatter(CkArgs c, const double* in, const int* recs, const int* scen,
                                                      int base, int count) {
  using T = typename CkUnit<U>::T;
  const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
  const long long r = (long long)blockIdx.x * wpb + (threadIdx.x >> 6);
  if (r < count) {
    const int sc = scen ? scen[r] : (int)r;
    const double* rec = in + (size_t)((recs ? recs[r] : (int)r) - base) * c.words;
    for (int x = lane * U; x < c.words; x += 64 * U) {
      const T t = *(const T*)(rec + x);
      double v[2] = {0.0, 0.0};
      memcpy(v, &t, sizeof(T));
      if ((unsigned)(x - c.ints_off) < (unsigned)CK_INT_WORDS) {
        for (int j = 0; j < U; ++j) {
          const int i0 = 2 * (x + j - c.ints_off);
          if (c.ints[i0]) c.ints[i0][sc] = __double2loint(v[j]);
          if (c.ints[i0 + 1]) c.ints[i0 + 1][sc] = __double2hiint(v[j]);
        }
      } else if (double* p = ck_word(c, sc, x)) {
        *(T*)p = t;
      }
    }
    if (lane == 0 && c.done) c.done[sc] = 0;
    if (lane == 0 && c.adv) c.adv[sc] = 0;
  }
}

}  // namespace

// ================================================================================================
// handle + C-ABI
// ================================================================================================
constexpr int DAT_MAX_SUB = 4;  // sub-batches of the C-ADMM closed loop (dat_set_sub_batches)
#ifndef DAT_STEP_PIPELINE_DEFAULT  // (A/B builds, tools/build_var.sh: -DDAT_STEP_PIPELINE_DEFAULT=false / true)
#define DAT_STEP_PIPELINE_DEFAULT true
#endif
#ifndef DAT_FUSED_ADVANCE_DEFAULT  // (likewise: -DDAT_FUSED_ADVANCE_DEFAULT=false / true)
#define DAT_FUSED_ADVANCE_DEFAULT true
#endif
#ifndef DAT_FUSED_SORT  // (A/B builds: 0 keeps k_bucket_adv behind k_advance)
#define DAT_FUSED_SORT 1
#endif
// The closed loop's log (dat_log_begin .. dat_log_end): device buffers filled by k_rollout_agents<true>, the log
// clock and what dat_log_clear has dropped.  Held records: HL clock / hl_every - hl_base, step
// ceil(clock / log_every) - step_base.
struct dat_log {
  bool open = false;
  int nslot = 0, log_every = 1, hl_cap = 0;
  long long step_cap = 0;
  int* slot = nullptr;
  double *hl = nullptr, *step = nullptr;
  int* sum_iters = nullptr;
  double* sum_mind = nullptr;
  unsigned char* sum_col = nullptr;
  long long clock = 0, hl_base = 0, step_base = 0;
  std::vector<double> hl_ms;  // per held HL record: device time of the step's control kernels (NaN: sub-batches)
  long long hl_count(int hl_every) const { return clock / hl_every - hl_base; }
  long long step_count() const { return (clock + log_every - 1) / log_every - step_base; }
};
// A side stream of the handle with its untimed events, made on first use, whole or not at all (side_get: st set
// means ready).  A stream made at dat_create would take one of the box's GPU_MAX_HW_QUEUES = 4 hardware queues
// from the sub-batch streams.
struct side_stream {
  hipStream_t st = nullptr;
  hipEvent_t ev[3] = {};
};
struct dat_handle {
  dat_log log;
  dat_config cfg;
  int P = 0, S = 0;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipEvent_t ek = nullptr;       // C-ADMM: after k_bucket
  double cadmm_ms = 0.0;         // summed device time of k_cadmm
  int persistent_blocks = 1024;  // C-ADMM: resident k_cadmm blocks (CUs x 4 wavefronts)
  double qp_tol = IPM_TOL;       // IPM stopping tolerance (dat_set_qp_tolerance)
  double* params = nullptr;
  int ppp = 0;
  bool have_params = false;
  double *state = nullptr, *acc = nullptr, *fdes = nullptr;
  int* counter = nullptr;
  double* trees = nullptr;
  int* tree_off = nullptr;
  int* scen_forest = nullptr;
  double* mountain = nullptr;
  int nforest = 0;
  double *cf = nullptr, *cfbar = nullptr, *clam = nullptr;
  int *rlist = nullptr, *rres = nullptr;  // C-ADMM: robust lists, resume records
  double *dlamF = nullptr, *dlamM = nullptr, *dprev = nullptr, *dHinv = nullptr;
  double* pf = nullptr;
  double* best = nullptr;
  int *iters = nullptr, *qstatus = nullptr;
  double *mind = nullptr, *err = nullptr;
  unsigned char* col = nullptr;
  unsigned long long* counters = nullptr;  // DAT_NCOUNTERS: [CNT_STRIDE k + .] of env class k (C-ADMM); [0..2] otherwise
  int *need = nullptr, *slist = nullptr, *scount = nullptr, *ipmx = nullptr;
  double* erows = nullptr;     // C-ADMM: env rows of the step, k_env_class -> k_cadmm
  unsigned* emask = nullptr;
  int env_sub = 0;             // sub-batches the last step's k_env_class ran on (the block layout of erows; 0: no step yet)
  long long hl_steps = 0;
  double hl_ms = 0.0;
  // host clock marks of the last dat_closed_loop call: its start, then each HL step's k_cadmm / k_dd /
  // k_cent completion (ms on a steady clock); consecutive differences are the per-step times of a
  // back-to-back run (dat_get_step_marks)
  std::vector<double> marks;
  double* acc_seq = nullptr;  // dat_control_steps: K x B x 6 desired accelerations (grown on demand)
  size_t acc_seq_cap = 0;
  double* pmrl_buf = nullptr;  // dat_pmrl_rollout: the force schedule (nf x B x 3n); dat_pmrl_forward: f and its outputs
  size_t pmrl_cap = 0;         // (grown on demand)
  // C-ADMM closed loop on sub-batches (dat_set_sub_batches): contiguous scenario ranges, each with its own
  // stream, so one sub-batch's kernels fill the drain tail and the short kernels of the others
  int nsub = 1;
  side_stream sub[DAT_MAX_SUB];    // [0].st: the handle's stream; ev[0]: the sub-batch's end, joined into that stream
  std::vector<hipEvent_t> sub_ev;  // dat_closed_loop on sub-batches: k_cadmm start / end events per step and sub-batch
  hipEvent_t ev_start = nullptr, ev_end = nullptr;
  // C-ADMM with a forest, one sub-batch: the tail-routed scenarios' launch beside k_cadmm, its start / end events
  side_stream tail;
  double* wrec = nullptr;  // C-ADMM: the tail's warm-start records (B n WREC_SIZE)
  // C-ADMM closed loop, one sub-batch, no log: the rollout and next env rows of the scenarios the drain has finished
  // run beside its ramp-down on a stream of their own (dat_closed_loop's overlap; dat_set_advance_overlap)
  bool adv_on = true;
  int serial = 0;                      // closed-loop steps of the handle so far: the step's stamp
  int *done = nullptr, *adv = nullptr;  // [B] stamps: KArgs::done, KArgs::adv
  int* qempty = nullptr;                // the mapped host word of KArgs::qempty, and its device address
  int* qempty_dev = nullptr;
  unsigned long long* advcnt = nullptr;  // KArgs::advcnt
  unsigned char* advmask = nullptr;      // dat_debug_advance_split: device copy of the mask (null: not set)
  side_stream advance;                   // the early pass's stream; ev[0]: its end, joined into the handle's stream
  // ... with the step pipeline (dat_set_step_pipeline): the early passes alternate between the advance stream and
  // this one, each followed on its stream by the next step's main drain.  ev[0]: the early pass's end; ev[1] / ev[2]
  // (on the handle's stream): after the rest chain's sort, after the rest drain.
  bool pipe_on = DAT_STEP_PIPELINE_DEFAULT;
  side_stream pipe;
  // the overlap's and the pipeline's passes (early, rest) as one launch each, k_advance, where a pass runs the
  // rollout and the next step's inputs (dat_set_fused_advance); off: the three kernels, same results
  bool fused_on = DAT_FUSED_ADVANCE_DEFAULT;
  mutable long long n_advance = 0, n_scatter = 0;  // launches of k_advance / k_bucket_scatter (dat_get_fused_launches)
  int* ktabs = nullptr;  // ... with the pipeline: the key tables of its sorts (4 x KT_INTS: main 0 / 1, rest 0 / 1)
  int* pipe_lists = nullptr;  // slist and rlist of the two pipeline streams' drains (4 x B; the handle's stream: slist, rlist)
  double agent_qp_ms = 0.0;  // device time of the last dat_solve_agent_qp_batch launch
  int ll_kind = 0;  // LL_PD (example/rqp_example.py:113) or LL_SM
  // dat_checkpoint_save / _load: the records' staging buffer and the index lists, grown on demand
  double* ck_stage = nullptr;
  int* ck_list = nullptr;
  size_t ck_stage_cap = 0, ck_list_cap = 0;
  double ck_kernel_ms = 0.0, ck_copy_ms = 0.0;  // device time of the last save's / load's copy kernel and host copy
  // what the handle owns: dat_destroy frees by list
  std::vector<void*> allocs;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> events;
};

// ---- the handle's per-scenario arrays --------------------------------------------------------------------------
// Every device array of the handle that holds a fixed number of elements per scenario, scenario-major, has its
// extent stated once: the checkpointed fp64 arrays in dat_ckpt.hpp (DAT_CK_FIELDS_*: words per scenario), the
// others here, per mode, as X(array, elements per scenario); the element type is the member's, and KArgs names
// its member like the handle.  dat_create's allocations, kargs' pointers and sub_kargs' views are written from
// these lists and from nothing else: a new array is one line here plus its two members.  Beyond the lists only
// the kernel that indexes an array knows its stride.  (counter and iters: the ints of a checkpoint record,
// DAT_CK_INT_FIELDS, which states no extent.  erows: SoA over the scenarios of a sub-batch, KArgs::erows.)
#define DAT_ARRAYS_ALL(X, n) X(counter, 1) X(iters, 1) X(acc, 6) X(qstatus, n) X(mind, 1) X(col, 1)
#define DAT_ARRAYS_CADMM(X, n)                                                              \
  X(need, 1) X(ipmx, 1) X(slist, 1) X(rlist, 1) X(done, 1) X(adv, 1) X(rres, RRES_INTS)     \
  X(erows, 4 * DAT_NENV * (n)) X(emask, n) X(wrec, (n) * WREC_SIZE) X(best, (n) * BEST_REC)
#define DAT_ARRAYS_DD(X, n)                                     \
  X(need, 1) X(ipmx, 1) X(slist, 1) X(dHinv, 36 * (n) * (n))    \
  X(wrec, (n) * WREC_SIZE) X(best, (n) * BEST_REC)
#define DAT_ARRAYS_CENT(X, n) X(best, NMAX_CENT * BEST_REC)
// Both lists of `mode` (a run-time value) through the caller's DAT_ARR(array, elements per scenario), a statement
#define DAT_ARR_CK(arr, words, off) DAT_ARR(arr, words)
#define DAT_ARRAYS_OF(mode, n)                \
  do {                                        \
    DAT_CK_FIELDS_OF(mode, DAT_ARR_CK, n);    \
    DAT_ARRAYS_ALL(DAT_ARR, n)                \
    if ((mode) == DAT_MODE_CADMM) {           \
      DAT_ARRAYS_CADMM(DAT_ARR, n)            \
    } else if ((mode) == DAT_MODE_DD) {       \
      DAT_ARRAYS_DD(DAT_ARR, n)               \
    } else {                                  \
      DAT_ARRAYS_CENT(DAT_ARR, n)             \
    }                                         \
  } while (0)

// C-ADMM scenario slots per k_cadmm wavefront: floor(64/n), fewer when the batch would not give
// every CU a wavefront.  A small batch is then spread one wavefront per CU (a wavefront's ADMM pass
// waits for the slowest of fewer lanes).  Not further: wavefronts sharing a CU pair's instruction
// cache at different points of the ~100 KB unrolled IPM slow each other down (C2, 1,024 scenarios,
// target blocks 1024 / 256 / 64 / floor(64/n) packing: 14.7 / 13.0 / 14.4 / 14.2 ms per step).
int cadmm_slots(const dat_handle* h, int B, int n) {
  const int gmax = 64 / n;
  int pb = h->persistent_blocks / 4 > 0 ? h->persistent_blocks / 4 : 1;
  const int g = (B + pb - 1) / pb;
  return g < 1 ? 1 : (g > gmax ? gmax : g);
}

namespace {

template <typename T>
int dalloc(dat_handle* h, T** p, size_t count) {
  *p = nullptr;
  if (count == 0) return 0;
  HIPCHK(hipMalloc((void**)p, count * sizeof(T)));
  HIPCHK(hipMemsetAsync(*p, 0, count * sizeof(T), h->stream));
  h->allocs.push_back(*p);
  return 0;
}

void dfree(dat_handle* h, void* p) {
  if (!p) return;
  for (auto& q : h->allocs)
    if (q == p) q = nullptr;
  (void)hipFree(p);
}

// err, the residual record (record_err handles only; dat_set_max_iter regrows it): elements per scenario
size_t err_extent(int max_iter) { return (size_t)max_iter + 1; }
// elements per scenario of the array behind the handle's member *member, as the lists state it
size_t extent_of(const dat_handle* h, const void* member) {
  size_t e = 0;
#define DAT_ARR(arr, per) \
  if ((const void*)&h->arr == member) e = (size_t)(per);
  DAT_ARRAYS_OF(h->cfg.mode, h->cfg.n);
#undef DAT_ARR
  return e;
}
// the scenarios [off, off + count) of sub-batch s of S: contiguous ranges that tile the batch
struct SubRange {
  int off, count;
};
SubRange sub_range(int batch, int s, int S) {
  const long long B = batch;
  const int off = (int)(B * s / S);
  return {off, (int)(B * (s + 1) / S) - off};
}

// a timed event of the handle's, made on first use
hipError_t own_event(dat_handle* h, hipEvent_t* e) {
  if (*e) return hipSuccess;
  const hipError_t r = hipEventCreate(e);
  if (r == hipSuccess) h->events.push_back(*e);
  return r;
}

// The side stream *s with nev events: got, or made on first use.  A failure leaves *s empty and no sticky error:
// the caller falls back (no tail routing, the serial schedule) or reports it.
hipError_t side_get(dat_handle* h, side_stream* s, int nev) {
  if (s->st) return hipSuccess;
  side_stream t;
  hipError_t e = hipStreamCreateWithFlags(&t.st, hipStreamNonBlocking);
  for (int k = 0; k < nev && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&t.ev[k], hipEventDisableTiming);
  if (e != hipSuccess) {
    for (hipEvent_t v : t.ev)
      if (v) (void)hipEventDestroy(v);
    if (t.st) (void)hipStreamDestroy(t.st);
    (void)hipGetLastError();
    return e;
  }
  h->streams.push_back(t.st);
  h->events.insert(h->events.end(), t.ev, t.ev + nev);
  *s = t;
  return hipSuccess;
}

// ... given back, after its work has ended (dat_set_sub_batches: a handle keeps no more streams than the four
// hardware queues it can count on); side_get makes it again on the next use
void side_release(dat_handle* h, side_stream* s) {
  if (!s->st) return;
  (void)hipStreamSynchronize(s->st);
  for (hipEvent_t v : s->ev) {
    if (!v) continue;
    h->events.erase(std::remove(h->events.begin(), h->events.end(), v), h->events.end());
    (void)hipEventDestroy(v);
  }
  h->streams.erase(std::remove(h->streams.begin(), h->streams.end(), s->st), h->streams.end());
  (void)hipStreamDestroy(s->st);
  *s = side_stream();
}

// The concurrent tail launch needs a stream of its own beside the step's: with sub-batches (4 streams) a fifth and
// more would share the hardware queues with them and serialise the sub-batches.
bool tail_wanted(const dat_handle* h) { return h->cfg.mode == DAT_MODE_CADMM && h->nforest > 0 && h->nsub == 1; }

// the handle as kernel arguments: a projection, nothing is created (the tail stream: step_entry)
KArgs kargs(const dat_handle* h) {
  KArgs a;
  memset(&a, 0, sizeof(a));
  const dat_config& c = h->cfg;
  a.B = c.batch;
  a.n = c.n;
  a.G = cadmm_slots(h, c.batch, c.n);
  a.P = h->P;
  a.S = h->S;
  a.ppp = h->ppp;
  // the per-scenario arrays, from the lists; those the mode does not have stay null
#define DAT_ARR(arr, per) a.arr = h->arr;
  DAT_ARRAYS_OF(c.mode, c.n);
#undef DAT_ARR
  a.done = a.adv = nullptr;  // the advance overlap's stamps are handed over where it runs (adv_args)
  a.params = h->params;
  a.trees = h->trees;
  a.tree_off = h->tree_off;
  a.scen_forest = h->scen_forest;
  a.nforest = h->nforest;
  a.mountain = h->mountain;
  a.max_iter = c.max_iter;
  a.res_tol = c.res_tol;
  a.use_total_res = c.use_total_res;
  a.rho0 = c.rho0;
  a.tau = c.tau_incr;
  a.rho_max = c.rho_max;
  a.record_err = c.record_err;
  a.qp_tol = h->qp_tol;
  a.ksteps = 1;
  a.err = h->err;
  a.counters = h->counters;
  a.scount = h->scount;
  a.ll_kind = h->ll_kind;
  a.tail_prev = h->nforest > 0 ? TAIL_PREV : INT_MAX;
  a.tail_pass = h->nforest > 0 ? TAIL_PASS : INT_MAX;
  a.route = tail_wanted(h) && h->tail.st;  // (no stream: the wedged scenarios go through k_cadmm's hand-over, same results)
  a.tmode = 0;
#ifdef DAT_NO_TAIL  // A/B builds only (tools/build_var.sh): the round-5 schedule, no tail rule
  a.tail_prev = a.tail_pass = INT_MAX;
  a.route = 0;
#endif
  return a;
}

size_t dd_lds(int n, bool env) { return dd_carve(nullptr, n, env).bytes(); }
size_t dd_setup_lds(int n) { return dd_setup_carve(nullptr, n).bytes(); }

// the C-ADMM drain of one control step: k_cadmm (env classes 3, 2, 1, 0) with a forest, k_cadmm0 without.
// k_cadmm_tail: one scenario slot per block (G = 1).  Its scenarios are few -- stalled ADMM loops next to trees,
// 101 sequential passes -- and a slot of its own per scenario keeps one scenario's pass from waiting for the
// slowest agent QP of the others'.  With a forest two launches: the tail-routed scenarios on the sub-batch's
// tail stream, started with k_cadmm (their lists are known after k_bucket), and the hand-over lists after
// k_cadmm on the step's stream, which then waits for the first.
constexpr int TAIL_BLOCKS = 256;
// (KArgs::done set: the ADV instantiations, dat_closed_loop's overlap)
int launch_cadmm(const dat_handle* h, const KArgs& a, int blocks, hipStream_t st) {
  KArgs r = a;
  r.G = 1;
  const bool adv = a.done != nullptr;
  const auto kc = adv ? k_cadmm<true> : k_cadmm<false>;
  const auto kt = k_cadmm_tail;
  const auto kc0 = adv ? k_cadmm0<true> : k_cadmm0<false>;
  const auto kt0 = k_cadmm0_tail;
  if (h->nforest > 0) {
    if (a.route) {
      KArgs t = r;
      t.tmode = 1;
      const hipStream_t ts = h->tail.st;
      HIPCHK(hipEventRecord(h->tail.ev[0], st));
      HIPCHK(hipStreamWaitEvent(ts, h->tail.ev[0], 0));
      hipLaunchKernelGGL(kt, dim3(TAIL_BLOCKS), dim3(64), cadmm_tail_lds_bytes(a.n, NCLS - 1), ts, t);
      HIPCHK(hipEventRecord(h->tail.ev[1], ts));
    }
    hipLaunchKernelGGL(kc, dim3(blocks), dim3(64), cadmm_lds_bytes(a.n, a.G, NCLS - 1), st, a);
    hipLaunchKernelGGL(kt, dim3(TAIL_BLOCKS), dim3(64), cadmm_tail_lds_bytes(r.n, NCLS - 1), st, r);
    if (a.route) HIPCHK(hipStreamWaitEvent(st, h->tail.ev[1], 0));
  } else {
    hipLaunchKernelGGL(kc0, dim3(blocks), dim3(64), cadmm_lds_bytes(a.n, a.G, 0), st, a);
    hipLaunchKernelGGL(kt0, dim3(TAIL_BLOCKS), dim3(64), cadmm_tail_lds_bytes(r.n, 0), st, r);
  }
  return 0;
}

// The DD kernels of a step: the quasi-Newton matrix (k_dd_setup<n>: [H | I] in registers to n = DD_REG_NMAX, <0>: in
// LDS, beyond the default 64 KB of dynamic LDS from n = 11 on), the sort by the previous step's iterations, the drain
int launch_dd(const dat_handle* h, const KArgs& a, hipStream_t st, hipEvent_t ek) {
  using K = void (*)(KArgs);
  static const K reg[] = {k_dd_setup<3>, k_dd_setup<4>, k_dd_setup<5>, k_dd_setup<6>, k_dd_setup<7>, k_dd_setup<8>};
  static_assert(DD_REG_NMAX == 8, "k_dd_setup<n>: one instantiation per n in [3, DD_REG_NMAX]");
  const int n = a.n, B = a.B;
  if (n > DD_REG_NMAX)
    HIPCHK(hipFuncSetAttribute((const void*)k_dd_setup<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)dd_setup_lds(n)));
  hipLaunchKernelGGL(n <= DD_REG_NMAX ? reg[n - 3] : k_dd_setup<0>, dim3(B), dim3(64), dd_setup_lds(n), st, a);
  hipLaunchKernelGGL(k_dd_key, dim3((B + 63) / 64), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_bucket, dim3(1), dim3(BUCKET_T), 0, st, B, (const int*)a.need, a.slist, a.scount);
  HIPCHK(hipEventRecord(ek, st));
  const bool env = h->nforest > 0;
  const int G = 64 / n, blocks = std::min((B + G - 1) / G, h->persistent_blocks);
  hipLaunchKernelGGL(env ? k_dd<true> : k_dd<false>, dim3(blocks), dim3(64), dd_lds(n, env), st, a);
  return 0;
}

// kernel arguments of sub-batch s, the scenarios r (dat_set_sub_batches; the whole batch: those of kargs): every
// per-scenario array offset by the lists' extents (the env-row image then a disjoint block of the SoA buffer,
// stride r.count n), the class table its own; counters shared (atomics)
template <class T>
T* offp(T* p, size_t k) { return p ? p + k : p; }
KArgs sub_kargs(const dat_handle* h, SubRange r, int s) {
  KArgs a = kargs(h);
  const size_t o = (size_t)r.off;
  a.B = r.count;
  a.G = cadmm_slots(h, r.count, a.n);
#define DAT_ARR(arr, per) a.arr = offp(a.arr, o * (size_t)(per));
  DAT_ARRAYS_OF(h->cfg.mode, a.n);
#undef DAT_ARR
  if (a.ppp) a.params += o * a.P;
  a.scen_forest = offp(a.scen_forest, o);
  a.err = offp(a.err, o * err_extent(a.max_iter));
  a.scount = h->scount + SCOUNT_INTS * s;
  return a;
}

// the open log's kernel arguments for the sub-batch of scenarios [off, ...) at the current clock
LogArgs log_args(const dat_handle* h, int off = 0) {
  const dat_log& g = h->log;
  LogArgs l;
  l.slot = g.slot + off;
  l.hl = g.hl;
  l.step = g.step;
  l.sum_iters = offp(g.sum_iters, (size_t)off);
  l.sum_mind = offp(g.sum_mind, (size_t)off);
  l.sum_col = offp(g.sum_col, (size_t)off);
  l.nslot = g.nslot;
  l.batch = h->cfg.batch;
  l.hl_every = h->cfg.hl_every;
  l.log_every = g.log_every;
  l.clock = g.clock;
  l.hl_base = g.hl_base;
  l.step_base = g.step_base;
  return l;
}

void log_free(dat_handle* h) {
  dat_log& g = h->log;
  for (void* p : {(void*)g.slot, (void*)g.hl, (void*)g.step, (void*)g.sum_iters, (void*)g.sum_mind, (void*)g.sum_col})
    (void)hipFree(p);
  g = dat_log();
}

// dat_closed_loop with a log open: the call must fit the HL capacity (nothing is dropped silently)
int log_admit(const dat_handle* h, int hl_steps) {
  const dat_log& g = h->log;
  if (!g.open || hl_steps <= 0) return 0;
  const long long held = g.hl_count(h->cfg.hl_every);
  if (held + hl_steps > g.hl_cap)
    return fail("dat_closed_loop: " + std::to_string(hl_steps) + " HL steps on top of the " + std::to_string(held) +
                " held would pass the log's hl_capacity = " + std::to_string(g.hl_cap) +
                " (read the log and dat_log_clear, or open it larger); nothing was run");
  return 0;
}

// ---- the step chain ------------------------------------------------------------------------------------------
// A control step is desired acceleration -> env rows and class keys -> class sort -> drain, and in the closed loop
// the rollout; each piece is stated once below, for one sub-batch.  dat_control_step, dat_control_steps and
// dat_closed_loop compose them.

// One sub-batch of a step: the scenarios [off, off + a.B) on their stream, and the event pair around their drain
// (ek after the sort, e1 after the control kernels).  The whole batch is the one sub-batch of S = 1.
struct Sub {
  hipStream_t st;
  KArgs a;
  int off;
  hipEvent_t ek, e1;
  // the step pipeline with the fused advance: the key tables (KeyTab) a pass's k_advance counts into (keys below
  // NKEY, tail-routed keys), the one a filtered sort reads and the one it zeroes; null: k_bucket_adv counts itself
  int *kc_lo = nullptr, *kc_hi = nullptr, *ktab = nullptr, *kzero = nullptr;
};
Sub sub_batch(const dat_handle* h, int s = 0, int S = 1) {
  const SubRange r = sub_range(h->cfg.batch, s, S);
  Sub u;
  u.st = h->sub[s].st;
  u.off = r.off;
  u.a = sub_kargs(h, r, s);
  u.ek = h->ek;
  u.e1 = h->e1;
  return u;
}
// ... with the closed loop's advance overlap switched on (one sub-batch: the whole batch)
void adv_args(const dat_handle* h, KArgs& a) {
  a.done = h->done;
  a.adv = h->adv;
  a.qempty = h->qempty_dev;
  a.advmask = h->advmask;
  a.advcnt = h->advcnt;
}

// What every entry point that runs control steps starts with.  The tail stream is made here, on first use.
int step_entry(dat_handle* h) {
  if (!h->have_params) return fail("dat_set_params has not been called");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (tail_wanted(h)) (void)side_get(h, &h->tail, 2);
  return 0;
}

// The inputs of a step for the scenarios of the pass `mode` (ADV_*, which picks the instantiations here): the
// desired acceleration, then (C-ADMM) the env rows and class keys.
enum { IN_DESIRED = 1, IN_ENV = 2 };
void launch_inputs(const dat_handle* h, const Sub& u, int mode = ADV_ALL, int parts = IN_DESIRED | IN_ENV) {
  struct Kernels {
    void (*desired)(KArgs, double*);
    void (*env_class)(KArgs);
  };
  static const Kernels ks[] = {{k_desired<ADV_ALL>, k_env_class<ADV_ALL>},
                               {k_desired<ADV_EARLY>, k_env_class<ADV_EARLY>},
                               {k_desired<ADV_REST>, k_env_class<ADV_REST>}};
  static_assert(ADV_ALL == 0 && ADV_EARLY == 1 && ADV_REST == 2, "ks is indexed by the mode");
  const int B = u.a.B, G = 64 / u.a.n;
  if (parts & IN_DESIRED)
    hipLaunchKernelGGL(ks[mode].desired, dim3((B + 63) / 64), dim3(64), 0, u.st, u.a, (double*)u.a.acc);
  if ((parts & IN_ENV) && h->cfg.mode == DAT_MODE_CADMM)
    hipLaunchKernelGGL(ks[mode].env_class, dim3((B + G - 1) / G), dim3(64), 0, u.st, u.a);
}

// the start of a step's timed span on one stream: the NaN pad of the residual record, e0
int step_begin(const dat_handle* h, const Sub& u) {
  if (h->cfg.record_err && u.a.err)
    HIPCHK(hipMemsetAsync(u.a.err, 0xff, sizeof(double) * (size_t)u.a.B * (h->cfg.max_iter + 1), u.st));
  HIPCHK(hipEventRecord(h->e0, u.st));
  return 0;
}

// The control kernels of the handle's mode, between the sub-batch's two events.  a.ksteps > 1 (dat_control_steps):
// that many control steps fused into one drain, a.acc ksteps x B x 6.
// C-ADMM, the step pipeline: `mode` ADV_EARLY / ADV_REST sorts and drains only the scenarios whose mark adv[] is /
// is not `stamp` (the previous step's serial).
int launch_control(const dat_handle* h, const Sub& u, int mode = ADV_ALL, int stamp = 0) {
  const KArgs& a = u.a;
  if (h->cfg.mode == DAT_MODE_CADMM) {  // the class sort of the step's keys (k_env_class), the drain
    if (mode == ADV_ALL)
      hipLaunchKernelGGL(k_bucket, dim3(1), dim3(BUCKET_T), 0, u.st, a.B, (const int*)a.need, a.slist, a.scount);
    else if (u.ktab) {
      hipLaunchKernelGGL(mode == ADV_EARLY ? k_bucket_scatter<ADV_EARLY> : k_bucket_scatter<ADV_REST>,
                         dim3((a.B + SCATTER_T - 1) / SCATTER_T), dim3(SCATTER_T), 0, u.st, a.B, (const int*)a.need,
                         a.slist, a.scount, (const int*)a.adv, stamp, u.ktab, u.kzero);
      ++h->n_scatter;
    } else
      hipLaunchKernelGGL(mode == ADV_EARLY ? k_bucket_adv<ADV_EARLY> : k_bucket_adv<ADV_REST>, dim3(1),
                         dim3(BUCKET_T), 0, u.st, a.B, (const int*)a.need, a.slist, a.scount, (const int*)a.adv, stamp);
    HIPCHK(hipEventRecord(u.ek, u.st));
    if (launch_cadmm(h, a, std::min((a.B + a.G - 1) / a.G, h->persistent_blocks), u.st)) return -1;
  } else if (h->cfg.mode == DAT_MODE_DD) {
    if (launch_dd(h, a, u.st, u.ek)) return -1;
  } else {
    HIPCHK(launch_cent(a.n, a.B, u.st, a));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(u.e1, u.st));
  return 0;
}

// a step from its desired accelerations on; timed: on one stream, with e0 in front (after k_desired)
int launch_step(const dat_handle* h, const Sub& u, bool timed = true) {
  if (timed && step_begin(h, u)) return -1;
  launch_inputs(h, u, ADV_ALL, IN_ENV);
  return launch_control(h, u);
}

// The rollout of a closed-loop step in the pass `mode`; with a log open the recording kernel, at the log's clock
// (sub-batch streams run unsynchronised: the record index is the sub-batch's own step count).
void launch_step_rollout(const dat_handle* h, const Sub& u, int mode = ADV_ALL) {
  const LogArgs lg = h->log.open ? log_args(h, u.off) : LogArgs();
  launch_rollout(u.a, u.a.B, u.st, h->cfg.hl_every, h->cfg.dt, (const double*)u.a.fdes, h->log.open ? &lg : nullptr,
                 mode);
}

// A pass (ADV_EARLY / ADV_REST) of the overlap and the pipeline: the rollout of the step and, with `inputs`, the next
// step's inputs of the scenarios it advanced.  One launch of k_advance where the switch is on (these schedules run
// C-ADMM on one sub-batch with no log open: advance_ready), else the three kernels of the step chain.
// fused_ready is the one statement of where k_advance runs: the passes go by it here, and the pipeline hands out key
// tables (Sub::kc_lo / ktab) by it, so a sort reads a key table only behind passes that counted into it.  A pass
// that is given a table and would not count (the three kernels do not) is an error, not a silently empty list.
bool fused_ready(const dat_handle* h) { return h->fused_on && h->cfg.mode == DAT_MODE_CADMM && !h->log.open; }
int launch_advance(const dat_handle* h, const Sub& u, int mode, bool inputs) {
  if (inputs && mode != ADV_ALL && fused_ready(h)) {
    const int G = 64 / u.a.n;
    hipLaunchKernelGGL(mode == ADV_EARLY ? k_advance<ADV_EARLY> : k_advance<ADV_REST>, dim3((u.a.B + G - 1) / G),
                       dim3(64), 0, u.st, u.a, h->cfg.hl_every, h->cfg.dt, (const double*)u.a.fdes, (double*)u.a.acc,
                       u.kc_lo, u.kc_hi);
    ++h->n_advance;
    return 0;
  }
  if (inputs && u.kc_lo) return fail("launch_advance: a key table was handed to a pass that runs the three kernels");
  launch_step_rollout(h, u, mode);
  if (inputs) launch_inputs(h, u, mode);
  return 0;
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The accounting of enqueued steps: waits for `end`; begin -> end is added to hl_ms, each of the ndrain pairs
// (after the sort, end of the control kernels) to cadmm_ms.  span_ms (optional): begin -> end.
int account(dat_handle* h, hipEvent_t begin, hipEvent_t end, const hipEvent_t* drain, size_t ndrain, int steps,
            double* span_ms = nullptr) {
  HIPCHK(hipEventSynchronize(end));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, begin, end));
  h->hl_ms += ms;
  if (span_ms) *span_ms = ms;
  for (size_t j = 0; j < ndrain; ++j) {
    float mk = 0.f;
    HIPCHK(hipEventElapsedTime(&mk, drain[2 * j], drain[2 * j + 1]));
    h->cadmm_ms += mk;
  }
  h->hl_steps += steps;
  return 0;
}
// ... of the ksteps control steps of one launch_step / launch_control on one stream (centralized: no drain span)
int account_step(dat_handle* h, const Sub& u, int ksteps = 1, double* step_ms = nullptr) {
  const hipEvent_t drain[2] = {u.ek, u.e1};
  return account(h, h->e0, u.e1, drain, h->cfg.mode != DAT_MODE_CENTRALIZED, ksteps, step_ms);
}

// a step's results, copied to the host arrays that are not null (on the handle's stream, not yet synchronised)
int copy_out(dat_handle* h, double* f_des, int* iters, int* qp_status, double* min_env_dist = nullptr,
             unsigned char* collision = nullptr, double* err_seq = nullptr) {
  const size_t B = h->cfg.batch, n = h->cfg.n;
  const hipStream_t st = h->stream;
  if (f_des) HIPCHK(hipMemcpyAsync(f_des, h->fdes, sizeof(double) * B * 3 * n, hipMemcpyDeviceToHost, st));
  if (iters) HIPCHK(hipMemcpyAsync(iters, h->iters, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  if (qp_status) HIPCHK(hipMemcpyAsync(qp_status, h->qstatus, sizeof(int) * B * n, hipMemcpyDeviceToHost, st));
  if (min_env_dist) HIPCHK(hipMemcpyAsync(min_env_dist, h->mind, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  if (collision) HIPCHK(hipMemcpyAsync(collision, h->col, B, hipMemcpyDeviceToHost, st));
  if (err_seq) {
    if (!h->err) return fail("dat_control_step: err_seq requested but record_err = 0");
    HIPCHK(hipMemcpyAsync(err_seq, h->err, sizeof(double) * B * (h->cfg.max_iter + 1), hipMemcpyDeviceToHost, st));
  }
  return 0;
}

// Does dat_closed_loop run the advance overlap?  C-ADMM on one sub-batch with no log open, the switch on, and the
// advance stream, its event and the host word in place (three streams with the tail's, within the four hardware
// queues).  Otherwise the serial schedule, same results.
bool advance_ready(dat_handle* h) {
  if (!h->adv_on || h->cfg.mode != DAT_MODE_CADMM || h->nsub != 1 || h->log.open) return false;
  if (!h->qempty || !h->qempty_dev || !h->done || !h->adv || !h->advcnt) return false;
  return side_get(h, &h->advance, 1) == hipSuccess;
}

// The overlap's host wait, after the drain of the step `serial` was enqueued: until the queue-empty word carries
// the serial, at the latest until the drain has ended (dat_debug_advance_split: always until then, so that every
// scenario's stamp is in place and the mask alone decides the split).
int wait_queue_empty(const dat_handle* h, int serial) {
  const volatile int* const qe = h->qempty;
  for (;;) {
    bool hit = false;
    for (int k = 0; k < 256 && !hit; ++k) hit = !h->advmask && *qe == serial;
    if (hit) break;
    const hipError_t q = hipEventQuery(h->e1);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) HIPCHK(q);
  }
  (void)hipGetLastError();  // (a not-ready query is no error of the loop's)
  return 0;
}

// the next closed-loop step's stamp (0: the arrays' initial value, no step's stamp)
int next_serial(dat_handle* h) { return h->serial = h->serial == INT_MAX ? 1 : h->serial + 1; }

// Does dat_closed_loop run the step pipeline?  Where the advance overlap runs, with the switch on, no residual
// record (its per-step pad is a whole-batch memset), and the second pipeline stream and the two further list sets
// in place: four streams with the tail's.  Otherwise the overlap schedule (or the serial one), same results.
bool pipeline_ready(dat_handle* h) {
  if (!h->pipe_on || h->cfg.record_err || !advance_ready(h)) return false;
  if (side_get(h, &h->pipe, 3) != hipSuccess) return false;
  if (!h->pipe_lists && dalloc(h, &h->pipe_lists, (size_t)4 * h->cfg.batch)) {
    (void)hipGetLastError();
    return false;
  }
  if (!h->ktabs && dalloc(h, &h->ktabs, (size_t)4 * KT_INTS)) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

// The closed loop as a step pipeline: per step two drains over disjoint scenarios.  The main drain of
// step k + 1 takes the scenarios the early pass of step k advanced and is enqueued directly behind that pass, on
// its stream: it starts beside step k's ramp-down and its workgroups are dispatched as the old ones retire.  The
// rest drain of step k + 1 takes the others, on the handle's stream, after both drains of step k have ended and the
// rest pass has advanced them.  What a drain reads of a scenario while the previous step's drains still run -- the
// warm state, plain stores of the drain that finished it -- has been written back by the kernel boundaries between
// the two (the early pass and the sort run after the stamp was seen); everything else it touches is the scenario's
// own and has one writer per step.  The early passes alternate between two streams, so that the pass of step k + 1
// does not queue behind the main drain of step k + 1.  Each of the three streams that run drains has its own
// class table and lists (a stream's drains are ordered, so a set is rewritten only after its last reader), and
// each step its own timed event pair.  The host never waits inside the loop: it polls the host word and queries
// events, and reads the spans at the end of the call.
int closed_loop_pipelined(dat_handle* h, int hl_steps) {
  const int B = h->cfg.batch;
  side_stream* const X[2] = {&h->advance, &h->pipe};
  while (h->sub_ev.size() < 2 * (size_t)hl_steps) {
    hipEvent_t e = nullptr;
    HIPCHK(own_event(h, &e));
    h->sub_ev.push_back(e);
  }
  Sub base = sub_batch(h);
  adv_args(h, base.a);
  // With the fused advance the passes count the keys of the sorts behind them (k_bucket_scatter).  The key tables of
  // the passes of step k: the main drain's `main(k)`, the rest drain's `rest(k)`, alternating with the step, each
  // zeroed by the sort of its kind one step earlier and all of them here, at the call's start (a call ends with the
  // last counting passes' tables sorted but not zeroed).
  const bool fsort = fused_ready(h) && DAT_FUSED_SORT;
  const auto main_tab = [&](int k) { return fsort ? h->ktabs + KT_INTS * (k & 1) : nullptr; };
  const auto rest_tab = [&](int k) { return fsort ? h->ktabs + KT_INTS * (2 + (k & 1)) : nullptr; };
  if (fsort) HIPCHK(hipMemsetAsync(h->ktabs, 0, sizeof(int) * 4 * KT_INTS, h->stream));
  // the main drain of step k: on the handle's stream over every scenario (k = 0, the first of the call), else on
  // the stream of the early pass it follows
  const auto main_drain = [&](int k, int serial) {
    Sub m = base;
    if (k > 0) {
      const int j = (k - 1) & 1;
      m.st = X[j]->st;
      m.a.slist = h->pipe_lists + (size_t)2 * j * B;
      m.a.rlist = m.a.slist + B;
      m.a.scount = h->scount + SCOUNT_INTS * (1 + j);  // (one sub-batch: the other sub-batches' tables are free)
      m.ktab = main_tab(k - 1);
      m.kzero = main_tab(k);
    }
    m.a.serial = serial;
    m.ek = h->sub_ev[2 * (size_t)k];
    m.e1 = h->sub_ev[2 * (size_t)k + 1];
    return m;
  };
  h->marks.assign(1, now_ms());
  int marked = 0;  // steps whose main drain the host has seen ended
  const auto mark = [&](int upto) {
    while (marked < upto && hipEventQuery(h->sub_ev[2 * (size_t)marked + 1]) == hipSuccess) {
      h->marks.push_back(now_ms());
      ++marked;
    }
    (void)hipGetLastError();  // (a not-ready query is no error of the loop's)
  };
  HIPCHK(hipEventRecord(h->e0, h->stream));
  launch_inputs(h, base);
  int serial = next_serial(h);
  if (launch_control(h, main_drain(0, serial))) return -1;
  for (int k = 0; k < hl_steps; ++k) {
    const bool more = k + 1 < hl_steps;
    const hipEvent_t e1 = h->sub_ev[2 * (size_t)k + 1];
    // until the main drain's class-0 queue has been claimed empty, at the latest until the drain has ended
    // (dat_debug_advance_split: always until then)
    for (const volatile int* const qe = h->qempty;;) {
      bool hit = false;
      for (int q = 0; q < 256 && !hit; ++q) hit = !h->advmask && *qe == serial;
      mark(k);
      if (hit) break;
      const hipError_t q = hipEventQuery(e1);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) HIPCHK(q);
    }
    (void)hipGetLastError();  // (a not-ready query is no error of the loop's)
    // the early pass of step k.  It marks adv[], which the rest chain of step k - 1 reads as its gate: after that
    // chain's sort.  With the split forced it also follows the rest drain of step k, for every stamp to be in place.
    side_stream& x = *X[k & 1];
    Sub early = base;
    early.st = x.st;
    early.a.serial = serial;
    early.kc_lo = main_tab(k);
    early.kc_hi = rest_tab(k);
    if (k > 0) HIPCHK(hipStreamWaitEvent(x.st, h->pipe.ev[1], 0));
    if (k > 0 && h->advmask) HIPCHK(hipStreamWaitEvent(x.st, h->pipe.ev[2], 0));
    if (launch_advance(h, early, ADV_EARLY, more)) return -1;
    HIPCHK(hipEventRecord(x.ev[0], x.st));
    const int next = more ? next_serial(h) : 0;
    if (more && launch_control(h, main_drain(k + 1, next), ADV_EARLY, serial)) return -1;
    // the rest chain of step k on the handle's stream (where the step's rest drain ran): after its main drain and
    // the early pass, the rest pass; then the sort and the drain of what it advanced.  That drain keeps the host
    // word out of it: its queue-empty store goes to a spare word of the class tables.
    Sub rest = base;
    rest.a.serial = serial;
    rest.kc_lo = rest.kc_hi = rest.ktab = rest_tab(k);
    rest.kzero = rest_tab(k + 1);
    if (k > 0) HIPCHK(hipStreamWaitEvent(rest.st, e1, 0));
    HIPCHK(hipStreamWaitEvent(rest.st, x.ev[0], 0));
    if (launch_advance(h, rest, ADV_REST, more)) return -1;
    if (more) {
      rest.a.serial = next;
      rest.a.qempty = h->scount + SCOUNT_INTS * 3;
      rest.ek = h->pipe.ev[1];
      rest.e1 = h->pipe.ev[2];
      if (launch_control(h, rest, ADV_REST, serial)) return -1;
    }
    HIPCHK(hipGetLastError());
    serial = next;
  }
  // the call's end: the handle's stream has joined the last main drain and early pass, and through them the others
  HIPCHK(hipEventRecord(h->e1, h->stream));
  HIPCHK(hipEventSynchronize(h->e1));
  for (side_stream* s : X) HIPCHK(hipStreamSynchronize(s->st));
  if (h->tail.st) HIPCHK(hipStreamSynchronize(h->tail.st));
  mark(hl_steps);
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
  h->hl_ms += ms;
  for (int k = 0; k < hl_steps; ++k) {  // (the main drains' spans: those of consecutive steps overlap)
    HIPCHK(hipEventElapsedTime(&ms, h->sub_ev[2 * (size_t)k], h->sub_ev[2 * (size_t)k + 1]));
    h->cadmm_ms += ms;
  }
  h->hl_steps += hl_steps;
  return 0;
}

// ---- the smaller shared pieces -------------------------------------------------------------------------------
// Temporary device buffers of one call, freed when the scope ends, on every path (hipFree waits for the device).
struct Scratch {
  std::vector<void*> held;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  ~Scratch() {
    for (void* p : held) (void)hipFree(p);
  }
  template <class T>
  T* get(size_t count) {  // (null when the allocation fails)
    void* p = nullptr;
    if (hipMalloc(&p, count ? count * sizeof(T) : 8) != hipSuccess) return nullptr;
    held.push_back(p);
    return (T*)p;
  }
};

// count words from src (the handle's counters; null: zeros), read after everything enqueued on the handle's stream
int read_words(dat_handle* h, const unsigned long long* src, unsigned long long* out, int count) {
  HIPCHK(hipSetDevice(h->cfg.device));
  std::fill(out, out + count, 0ull);
  if (!src) return 0;
  HIPCHK(hipMemcpyAsync(out, src, sizeof(*out) * count, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
// ... each word to its destination, where that is not null
int read_words(dat_handle* h, const unsigned long long* src, std::initializer_list<long long*> out) {
  unsigned long long c[8];
  if (read_words(h, src, c, (int)out.size())) return -1;
  int k = 0;
  for (long long* p : out) {
    if (p) *p = (long long)c[k];
    ++k;
  }
  return 0;
}

// ---- checkpoints ---------------------------------------------------------------------------------------------
// the handle's record as the copy kernels' arguments: the table of dat_ckpt.hpp with the handle's arrays put in
CkArgs ck_args(const dat_handle* h) {
  CkArgs c;
  memset(&c, 0, sizeof(c));
  const int n = h->cfg.n;
#define DAT_CK_X(arr, w_, o_) \
  c.f[c.nf] = h->arr;         \
  c.w[c.nf] = (w_);           \
  c.off[c.nf] = (o_);         \
  ++c.nf;
  DAT_CK_FIELDS_OF(h->cfg.mode, DAT_CK_X, n);
#undef DAT_CK_X
#define DAT_CK_X(arr, k) c.ints[k] = h->arr;
  DAT_CK_INT_FIELDS(DAT_CK_X)
#undef DAT_CK_X
  c.ints_off = DAT_CK_INTS(n);
  c.words = ck_record_words(h->cfg.mode, n);
  c.done = h->done;
  c.adv = h->adv;
  return c;
}
// 16-byte units where every segment's words and offset are even (kernels: CkUnit)
bool ck_wide(const CkArgs& c) {
  bool even = c.ints_off % 2 == 0 && c.words % 2 == 0;
  for (int k = 0; k < c.nf; ++k) even = even && c.w[k] % 2 == 0 && c.off[k] % 2 == 0;
  return even;
}
int ck_blocks(int count) { return (int)(((long long)count + 3) / 4); }  // (four wavefronts, one record each, per block)

// the spans of a save / load (events of the handle's, recorded on its stream and reached): its kernel, its host copy
int ck_times(dat_handle* h, hipEvent_t k0, hipEvent_t k1, hipEvent_t c0, hipEvent_t c1) {
  float km = 0.f, cm = 0.f;
  HIPCHK(hipEventElapsedTime(&km, k0, k1));
  HIPCHK(hipEventElapsedTime(&cm, c0, c1));
  h->ck_kernel_ms = km;
  h->ck_copy_ms = cm;
  return 0;
}

// A buffer of the handle's grown to `need` elements (not cleared: every word read was written before).  A failure
// leaves the old buffer in place.
template <class T>
int ck_grow(dat_handle* h, T** p, size_t* cap, size_t need) {
  if (need <= *cap) return 0;
  void* q = nullptr;
  const hipError_t e = hipMalloc(&q, need * sizeof(T));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(std::string("checkpoint staging buffer: ") + hipGetErrorString(e));
  }
  dfree(h, *p);
  h->allocs.push_back(q);
  *p = (T*)q;
  *cap = need;
  return 0;
}

}  // namespace

extern "C" {

#ifdef DAT_CAPTURE_LOOSE
int dat_get_captures(double* out, int* count) {
  HIPCHK(hipDeviceSynchronize());
  unsigned int k = 0;
  HIPCHK(hipMemcpyFromSymbol(&k, HIP_SYMBOL(dat::g_ncap), sizeof(k)));
  *count = (int)k;
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(dat::g_cap), sizeof(double) * CAP_MAX * CAP_DOUBLES));
  return 0;
}
#endif
#ifdef DAT_ITER_HIST
int dat_get_iter_hist(unsigned long long* out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(dat::g_iter_hist), sizeof(unsigned long long) * 64));
  unsigned long long z[64] = {0};
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(dat::g_iter_hist), z, sizeof(z)));
  return 0;
}
#endif
#ifdef DAT_PHASE_PROF
// development builds only (tools/phase_prof.py): the IPM phase cycle sums, reset after the read
int dat_get_phase_cycles(unsigned long long* out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(dat::g_phase), sizeof(unsigned long long) * 16));
  unsigned long long z[16] = {0};
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(dat::g_phase), z, sizeof(z)));
  return 0;
}
#endif

void dat_default_config(dat_config* c) {
  memset(c, 0, sizeof(*c));
  c->device = 0;
  c->mode = DAT_MODE_CADMM;
  c->n = 3;
  c->batch = 1;
  c->dt = 1e-3;
  c->hl_every = 10;
  c->max_iter = 100;
  c->res_tol = 1e-2;
  c->use_total_res = 1;
  c->rho0 = 1.0;
  c->tau_incr = 1.0;
  c->rho_max = 2.0;
  c->record_err = 0;
}

const char* dat_last_error(void) { return g_err.c_str(); }

int dat_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int dat_create(const dat_config* cfg, dat_handle** out) {
  if (!cfg || !out) return fail("dat_create: null argument");
  *out = nullptr;
  const dat_config& c = *cfg;
  if (c.n < 3 || c.n > NMAX) return fail("dat_create: n must be in [3, 16]");
  if (c.mode == DAT_MODE_DD && c.n > NMAX_DD) return fail("dat_create: DD supports n <= 16");
  if (c.mode == DAT_MODE_CENTRALIZED && c.n > NMAX_CENT) return fail("dat_create: centralized supports n <= 16");
  if (c.mode < 0 || c.mode > 2) return fail("dat_create: bad mode");
  if (c.batch < 1) return fail("dat_create: batch must be >= 1");
  if (c.max_iter < 0) return fail("dat_create: max_iter must be >= 0");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (c.device < 0 || c.device >= ndev) return fail("dat_create: no such HIP device");
  HIPCHK(hipSetDevice(c.device));
  dat_handle* h = new dat_handle();
  h->cfg = c;
  h->P = DAT_PARAM_SIZE(c.n);
  h->S = DAT_STATE_SIZE(c.n);
  // (the side streams are made on first use, side_get)
  hipError_t ce = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (ce == hipSuccess) h->streams.push_back(h->stream);
  for (hipEvent_t* e : {&h->e0, &h->e1, &h->ek})
    if (ce == hipSuccess) ce = own_event(h, e);
  if (ce != hipSuccess) {
    dat_destroy(h);
    return fail("dat_create: stream/event creation failed");
  }
  h->sub[0].st = h->stream;
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c.device) == hipSuccess && ncu > 0)
    h->persistent_blocks = 4 * ncu;  // k_cadmm: one wavefront per SIMD (register-bound), 4 SIMDs per CU
  const size_t B = c.batch;
  int rc = 0;
  // the per-scenario arrays of the mode, from the lists
#define DAT_ARR(arr, per) rc |= dalloc(h, &h->arr, B * (size_t)(per));
  DAT_ARRAYS_OF(c.mode, c.n);
#undef DAT_ARR
  if (c.record_err) rc |= dalloc(h, &h->err, B * err_extent(c.max_iter));
  // the others: the counters, the queues' class tables (C-ADMM: one per sub-batch), the advance overlap's words
  rc |= dalloc(h, &h->counters, DAT_NCOUNTERS);
  if (c.mode != DAT_MODE_CENTRALIZED)
    rc |= dalloc(h, &h->scount, SCOUNT_INTS * (c.mode == DAT_MODE_CADMM ? DAT_MAX_SUB : 1));
  if (c.mode == DAT_MODE_CADMM) {
    rc |= dalloc(h, &h->advcnt, 2);
    // (without the host word the closed loop keeps the serial schedule)
    if (hipHostMalloc((void**)&h->qempty, sizeof(int), hipHostMallocMapped) == hipSuccess) {
      *h->qempty = 0;
      if (hipHostGetDevicePointer((void**)&h->qempty_dev, h->qempty, 0) != hipSuccess) h->qempty_dev = nullptr;
    } else {
      h->qempty = nullptr;
      (void)hipGetLastError();
    }
  }
  if (rc || dat_reset_counters(h)) {
    std::string m = g_err;
    dat_destroy(h);
    return fail(m);
  }
  if (c.mode == DAT_MODE_CADMM) {  // the tail's workgroup may exceed the default 64 KB of dynamic LDS
    // The limit belongs to the kernel (per device), not to the handle: it is only ever raised, so a handle
    // of a smaller team created later never lowers it under a live handle of a larger one.
    static std::mutex mu;
    static int cur[64] = {0};
    const int tl = (int)cadmm_tail_lds_bytes(c.n);
    std::lock_guard<std::mutex> lk(mu);
    int* have = c.device >= 0 && c.device < 64 ? &cur[c.device] : nullptr;
    if (!have || tl > *have) {
      if (hipFuncSetAttribute((const void*)k_cadmm_tail, hipFuncAttributeMaxDynamicSharedMemorySize, tl) != hipSuccess ||
          hipFuncSetAttribute((const void*)k_cadmm0_tail, hipFuncAttributeMaxDynamicSharedMemorySize, tl) != hipSuccess) {
        dat_destroy(h);
        return fail("dat_create: tail kernel LDS attribute");
      }
      if (have) *have = tl;
    }
  }
  // LDS budgets
  size_t lds = c.mode == DAT_MODE_CADMM ? cadmm_lds_bytes(c.n, 64 / c.n) : (c.mode == DAT_MODE_DD ? dd_setup_lds(c.n) : 0);
  if (lds > 160 * 1024) {
    dat_destroy(h);
    return fail("dat_create: LDS budget exceeded");
  }
  *out = h;
  return 0;
}

int dat_destroy(dat_handle* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->cfg.device);
  for (hipStream_t s : h->streams) (void)hipStreamSynchronize(s);
  for (void* p : h->allocs)
    if (p) (void)hipFree(p);
  log_free(h);
  if (h->qempty) (void)hipHostFree(h->qempty);
  for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
  for (hipStream_t s : h->streams) (void)hipStreamDestroy(s);
  delete h;
  return 0;
}

int dat_set_params(dat_handle* h, const double* params, int per_scenario) {
  if (!h || !params) return fail("dat_set_params: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  size_t count = (per_scenario ? (size_t)h->cfg.batch : 1) * h->P;
  if (h->params) dfree(h, h->params);
  if (dalloc(h, &h->params, count)) return -1;
  HIPCHK(hipMemcpyAsync(h->params, params, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
  h->ppp = per_scenario ? 1 : 0;
  h->have_params = true;
  return dat_reset_warm_start(h);
}

int dat_set_forests(dat_handle* h, int num_forests, const int* tree_offsets, const double* tree_pos,
                    const int* scenario_forest, const double* mountain) {
  if (!h) return fail("dat_set_forests: null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  dfree(h, h->trees);
  dfree(h, h->tree_off);
  dfree(h, h->scen_forest);
  dfree(h, h->mountain);
  h->trees = nullptr;
  h->tree_off = nullptr;
  h->scen_forest = nullptr;
  h->mountain = nullptr;
  h->nforest = 0;
  if (num_forests <= 0) return 0;
  if (!tree_offsets || !tree_pos) return fail("dat_set_forests: null forest data");
  const int T = tree_offsets[num_forests];
  if (T < 0) return fail("dat_set_forests: bad offsets");
  for (int f = 0; f < num_forests; ++f)
    if (tree_offsets[f + 1] < tree_offsets[f]) return fail("dat_set_forests: offsets must be non-decreasing");
  if (dalloc(h, &h->trees, (size_t)(T > 0 ? T : 1) * 3) || dalloc(h, &h->tree_off, num_forests + 1)) return -1;
  if (T > 0) {
    // each forest's trees sorted by x: env_rows scans only the x-window of its vision range
    std::vector<double> sorted((size_t)3 * T);
    std::vector<int> idx;
    for (int f = 0; f < num_forests; ++f) {
      const int b = tree_offsets[f], e = tree_offsets[f + 1];
      idx.resize(e - b);
      for (int k = 0; k < e - b; ++k) idx[k] = b + k;
      std::stable_sort(idx.begin(), idx.end(), [&](int u, int v) { return tree_pos[3 * u] < tree_pos[3 * v]; });
      for (int k = 0; k < e - b; ++k)
        for (int c = 0; c < 3; ++c) sorted[(size_t)3 * (b + k) + c] = tree_pos[(size_t)3 * idx[k] + c];
    }
    HIPCHK(hipMemcpyAsync(h->trees, sorted.data(), sizeof(double) * 3 * T, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  HIPCHK(hipMemcpyAsync(h->tree_off, tree_offsets, sizeof(int) * (num_forests + 1), hipMemcpyHostToDevice, h->stream));
  if (scenario_forest) {
    for (int s = 0; s < h->cfg.batch; ++s)
      if (scenario_forest[s] >= num_forests) return fail("dat_set_forests: scenario_forest out of range");
    if (dalloc(h, &h->scen_forest, h->cfg.batch)) return -1;
    HIPCHK(hipMemcpyAsync(h->scen_forest, scenario_forest, sizeof(int) * h->cfg.batch, hipMemcpyHostToDevice, h->stream));
  }
  if (mountain) {
    if (dalloc(h, &h->mountain, (size_t)num_forests * DAT_MOUNTAIN_SIZE)) return -1;
    HIPCHK(hipMemcpyAsync(h->mountain, mountain, sizeof(double) * num_forests * DAT_MOUNTAIN_SIZE, hipMemcpyHostToDevice,
                          h->stream));
  }
  h->nforest = num_forests;
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_set_tolerance(dat_handle* h, double res_tol, int use_total_res) {
  if (!h) return fail("null handle");
  h->cfg.res_tol = res_tol;
  h->cfg.use_total_res = use_total_res;
  return 0;
}

int dat_set_qp_tolerance(dat_handle* h, double tol) {
  if (!h) return fail("null handle");
  if (!(tol >= 1e-12 && tol <= 1e-7)) return fail("dat_set_qp_tolerance: tol must lie in [1e-12, 1e-7]");
  h->qp_tol = tol;
  return 0;
}

int dat_set_max_iter(dat_handle* h, int max_iter) {
  if (!h) return fail("null handle");
  if (max_iter < 0) return fail("dat_set_max_iter: negative");
  if (h->cfg.record_err && max_iter > h->cfg.max_iter) {
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    dfree(h, h->err);
    h->err = nullptr;
    if (dalloc(h, &h->err, (size_t)h->cfg.batch * err_extent(max_iter))) return -1;
  }
  h->cfg.max_iter = max_iter;
  return 0;
}

int dat_reset_warm_start(dat_handle* h) {
  if (!h) return fail("null handle");
  if (!h->have_params) return fail("dat_reset_warm_start: params not set");
  HIPCHK(hipSetDevice(h->cfg.device));
  KArgs a = kargs(h);
  hipLaunchKernelGGL(k_warm, dim3((h->cfg.batch + 63) / 64), dim3(64), 0, h->stream, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_set_state(dat_handle* h, const double* state, const int* counters) {
  if (!h || !state) return fail("dat_set_state: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpyAsync(h->state, state, sizeof(double) * (size_t)h->cfg.batch * h->S, hipMemcpyHostToDevice, h->stream));
  if (counters)
    HIPCHK(hipMemcpyAsync(h->counter, counters, sizeof(int) * h->cfg.batch, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_get_state(dat_handle* h, double* state, int* counters) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (state)
    HIPCHK(hipMemcpyAsync(state, h->state, sizeof(double) * (size_t)h->cfg.batch * h->S, hipMemcpyDeviceToHost, h->stream));
  if (counters)
    HIPCHK(hipMemcpyAsync(counters, h->counter, sizeof(int) * h->cfg.batch, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_checkpoint_bytes(dat_handle* h, int count, long long* bytes) {
  if (!h || !bytes) return fail("dat_checkpoint_bytes: null argument");
  if (count < 0) return fail("dat_checkpoint_bytes: negative count " + std::to_string(count));
  *bytes = ck_blob_bytes(h->cfg.mode, h->cfg.n, count);
  return 0;
}

int dat_checkpoint_save(dat_handle* h, const int* scenarios, int count, void* blob, long long bytes) {
  if (!h) return fail("dat_checkpoint_save: null handle");
  std::string m;
  if (ck_check_save(h->cfg.mode, h->cfg.n, h->cfg.batch, scenarios, count, blob, bytes, &m)) return fail(m);
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t s : h->streams) HIPCHK(hipStreamSynchronize(s));
  ck_put_header(blob, h->cfg.mode, h->cfg.n, count);
  if (count == 0) return 0;
  const CkArgs c = ck_args(h);
  const size_t words = (size_t)count * c.words;
  if (ck_grow(h, &h->ck_stage, &h->ck_stage_cap, words)) return -1;
  if (scenarios) {
    if (ck_grow(h, &h->ck_list, &h->ck_list_cap, (size_t)count)) return -1;
    HIPCHK(hipMemcpyAsync(h->ck_list, scenarios, sizeof(int) * count, hipMemcpyHostToDevice, h->stream));
  }
  const int* list = scenarios ? h->ck_list : nullptr;
  HIPCHK(hipEventRecord(h->e0, h->stream));
  hipLaunchKernelGGL(ck_wide(c) ? k_ckpt_gather<2> : k_ckpt_gather<1>, dim3(ck_blocks(count)), dim3(256), 0, h->stream, c,
                     list, count, h->ck_stage);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ek, h->stream));
  HIPCHK(hipMemcpyAsync((char*)blob + DAT_CK_HEADER_BYTES, h->ck_stage, sizeof(double) * words, hipMemcpyDeviceToHost,
                        h->stream));
  HIPCHK(hipEventRecord(h->e1, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return ck_times(h, h->e0, h->ek, h->ek, h->e1);
}

int dat_checkpoint_load(dat_handle* h, const void* blob, long long bytes, const int* records, const int* scenarios,
                        int count) {
  if (!h) return fail("dat_checkpoint_load: null handle");
  std::string m;
  long long lo = 0, hi = 0;
  if (ck_check_load(h->cfg.mode, h->cfg.n, h->cfg.batch, blob, bytes, records, scenarios, count, &lo, &hi, &m))
    return fail(m);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t s : h->streams) HIPCHK(hipStreamSynchronize(s));
  const CkArgs c = ck_args(h);
  // the records named lie in [lo, hi) of the blob: that stretch is uploaded, once
  const size_t words = (size_t)(hi - lo) * c.words;
  if (ck_grow(h, &h->ck_stage, &h->ck_stage_cap, words) || ck_grow(h, &h->ck_list, &h->ck_list_cap, (size_t)2 * count))
    return -1;
  const hipStream_t st = h->stream;
  HIPCHK(hipEventRecord(h->e0, st));
  HIPCHK(hipMemcpyAsync(h->ck_stage, (const char*)blob + DAT_CK_HEADER_BYTES + sizeof(double) * (size_t)lo * c.words,
                        sizeof(double) * words, hipMemcpyHostToDevice, st));
  int *recs = nullptr, *scen = nullptr;
  if (records) {
    recs = h->ck_list;
    HIPCHK(hipMemcpyAsync(recs, records, sizeof(int) * count, hipMemcpyHostToDevice, st));
  }
  if (scenarios) {
    scen = h->ck_list + count;
    HIPCHK(hipMemcpyAsync(scen, scenarios, sizeof(int) * count, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipEventRecord(h->ek, st));
  hipLaunchKernelGGL(ck_wide(c) ? k_ckpt_scatter<2> : k_ckpt_scatter<1>, dim3(ck_blocks(count)), dim3(256), 0, st, c,
                     (const double*)h->ck_stage, (const int*)recs, (const int*)scen, (int)lo, count);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->e1, st));
  HIPCHK(hipStreamSynchronize(st));
  return ck_times(h, h->ek, h->e1, h->e0, h->ek);
}

int dat_get_checkpoint_ms(dat_handle* h, double* kernel_ms, double* copy_ms) {
  if (!h) return fail("dat_get_checkpoint_ms: null handle");
  if (kernel_ms) *kernel_ms = h->ck_kernel_ms;
  if (copy_ms) *copy_ms = h->ck_copy_ms;
  return 0;
}

int dat_control_step(dat_handle* h, const double* state, const double* acc_des, double* f_des, int* iters,
                     int* qp_status, double* min_env_dist, unsigned char* collision, double* err_seq) {
  if (!h) return fail("null handle");
  if (step_entry(h)) return -1;
  const size_t B = h->cfg.batch;
  if (state) HIPCHK(hipMemcpyAsync(h->state, state, sizeof(double) * B * h->S, hipMemcpyHostToDevice, h->stream));
  const Sub u = sub_batch(h);
  h->env_sub = 1;
  if (acc_des) {
    HIPCHK(hipMemcpyAsync(h->acc, acc_des, sizeof(double) * B * 6, hipMemcpyHostToDevice, h->stream));
  } else {
    launch_inputs(h, u, ADV_ALL, IN_DESIRED);
    HIPCHK(hipGetLastError());
  }
  if (launch_step(h, u)) return -1;
  if (copy_out(h, f_des, iters, qp_status, min_env_dist, collision, err_seq)) return -1;
  if (account_step(h, u)) return -1;
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_control_steps(dat_handle* h, int steps, const double* acc_seq, double* f_des, int* iters, int* qp_status) {
  if (!h || !acc_seq) return fail("dat_control_steps: null argument");
  if (steps <= 0) return fail("dat_control_steps: steps must be >= 1");
  if (h->cfg.mode != DAT_MODE_CADMM && h->cfg.mode != DAT_MODE_DD)
    return fail("dat_control_steps: C-ADMM and DD handles only");
  if (h->nforest > 0) return fail("dat_control_steps: handles without a forest only (env rows change with the state)");
  if (h->cfg.record_err) return fail("dat_control_steps: record_err must be 0");
  if (step_entry(h)) return -1;
  const size_t need = (size_t)steps * h->cfg.batch * 6;
  if (need > h->acc_seq_cap) {
    dfree(h, h->acc_seq);
    h->acc_seq_cap = 0;
    if (dalloc(h, &h->acc_seq, need)) return -1;
    h->acc_seq_cap = need;
  }
  HIPCHK(hipMemcpyAsync(h->acc_seq, acc_seq, sizeof(double) * need, hipMemcpyHostToDevice, h->stream));
  Sub u = sub_batch(h);
  h->env_sub = 1;
  u.a.ksteps = steps;
  u.a.acc = h->acc_seq;
  if (launch_step(h, u)) return -1;
  if (copy_out(h, f_des, iters, qp_status)) return -1;
  if (account_step(h, u, steps)) return -1;
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_rollout(dat_handle* h, int steps, const double* f_des) {
  if (!h) return fail("null handle");
  if (steps <= 0) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = h->cfg.batch, n = h->cfg.n;
  if (f_des) HIPCHK(hipMemcpyAsync(h->fdes, f_des, sizeof(double) * B * 3 * n, hipMemcpyHostToDevice, h->stream));
  if (!h->have_params) return fail("dat_rollout: params not set");
  KArgs a = kargs(h);
  launch_rollout(a, (int)B, h->stream, steps, h->cfg.dt, (const double*)h->fdes);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// The closed loop: hl_steps x (desired acceleration, env rows and keys, control kernels, rollout), in one of four
// schedules of the same step chain.
//   serial       one sub-batch on the handle's stream; the host waits for each step's control kernels (the rollout
//                still runs while the next step is enqueued).
//   sub-batches  S of them, each on its own stream, no synchronisation between the sub-batches or the steps; the
//                host waits once, for the call's end.
//   overlap      (advance_ready) the serial chain with the rollout and the next step's inputs split into two passes
//                over disjoint scenarios: `early` on the advance stream beside the drain's ramp-down, on the
//                scenarios whose done stamp is the step's, started when k_cadmm's class-0 queue has been claimed
//                empty (the host word) or the drain has ended; `rest` on the handle's stream after the drain, on the
//                others.  A scenario's step is the same sequence of the same device functions on the same inputs in
//                either pass.  The inputs of a call's first step are computed for every scenario up front, and none
//                after its last step (the next call starts from the state alone, which dat_set_state may replace).
//   pipeline     (pipeline_ready; closed_loop_pipelined) the overlap with the next step's drain split likewise: the
//                scenarios the early pass has advanced are sorted and drained directly behind it, beside the current
//                drain's ramp-down, the others after the rest pass.
// What the early pass may touch while the drain runs: a finished scenario's state, acc, env rows / mask, sort key
// and rotation counter are read by the drain only when a slot takes the scenario (the refill; ksteps == 1 here),
// so they may be overwritten; its f_des, iters and ipmx were stored write-through before the stamp and are read
// past the caches; everything else the early kernels read dates from before the drain's launch.
// With sub-batches hl_ms is the whole call's device time (the sub-batches' kernels overlap) and cadmm_ms the sum of
// the k_cadmm launch spans (S launches per HL step: dat_get_kernel_ms / (hl_steps S) is one launch).
int dat_closed_loop(dat_handle* h, int hl_steps) {
  if (!h) return fail("null handle");
  if (log_admit(h, hl_steps) || step_entry(h)) return -1;
  const int S = h->nsub;
  if (hl_steps > 0) h->env_sub = S;
  if (hl_steps > 0 && pipeline_ready(h)) return closed_loop_pipelined(h, hl_steps);
  const bool overlap = advance_ready(h);
  const size_t ndrain = S > 1 && hl_steps > 0 ? (size_t)S * hl_steps : 0;
  Sub u[DAT_MAX_SUB];
  for (int s = 0; s < S; ++s) u[s] = sub_batch(h, s, S);
  if (overlap) adv_args(h, u[0].a);
  h->marks.assign(1, now_ms());
  if (S > 1) {  // a drain event pair per step and sub-batch; the sub-batch streams start after the handle's
    while (h->sub_ev.size() < 2 * ndrain) {
      hipEvent_t e = nullptr;
      HIPCHK(own_event(h, &e));
      h->sub_ev.push_back(e);
    }
    HIPCHK(hipEventRecord(h->ev_start, h->stream));
    for (int s = 1; s < S; ++s) HIPCHK(hipStreamWaitEvent(u[s].st, h->ev_start, 0));
  }
  for (int k = 0; k < hl_steps; ++k) {
    for (int s = 0; s < S; ++s) {
      Sub& v = u[s];
      if (S > 1) {
        v.ek = h->sub_ev[2 * ((size_t)k * S + s)];
        v.e1 = h->sub_ev[2 * ((size_t)k * S + s) + 1];
      }
      if (!overlap) {
        launch_inputs(h, v, ADV_ALL, IN_DESIRED);
        if (launch_step(h, v, S == 1)) return -1;
        launch_step_rollout(h, v);
      } else {
        if (step_begin(h, v)) return -1;
        if (k == 0) launch_inputs(h, v);
        v.a.serial = next_serial(h);
        if (launch_control(h, v) || wait_queue_empty(h, h->serial)) return -1;
        // the passes after the drain: the rollout, then (not after the call's last step) the next step's inputs
        Sub early = v;
        early.st = h->advance.st;
        if (launch_advance(h, early, ADV_EARLY, k + 1 < hl_steps)) return -1;
        HIPCHK(hipEventRecord(h->advance.ev[0], early.st));
        // (the rest pass is enqueued before the wait for the drain, so that its end finds it in the queue)
        HIPCHK(hipStreamWaitEvent(v.st, h->advance.ev[0], 0));
        if (launch_advance(h, v, ADV_REST, k + 1 < hl_steps)) return -1;
      }
      HIPCHK(hipGetLastError());
    }
    double step_ms = std::nan("");  // no per-step time is defined on overlapping streams
    if (S == 1 && account_step(h, u[0], 1, &step_ms)) return -1;
    if (h->log.open) {
      h->log.clock += h->cfg.hl_every;
      h->log.hl_ms.push_back(step_ms);
    }
    if (S == 1) h->marks.push_back(now_ms());
  }
  if (S > 1) {
    for (int s = 1; s < S; ++s) {
      HIPCHK(hipEventRecord(h->sub[s].ev[0], u[s].st));
      HIPCHK(hipStreamWaitEvent(h->stream, h->sub[s].ev[0], 0));
    }
    HIPCHK(hipEventRecord(h->ev_end, h->stream));
    if (account(h, h->ev_start, h->ev_end, h->sub_ev.data(), ndrain, hl_steps)) return -1;
    h->marks.push_back(now_ms());
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_get_refinement_counters(dat_handle* h, long long* passes, long long* corrections) {
  if (!h) return fail("null handle");
  return read_words(h, h->counters + CNT_REF, {passes, corrections});
}

int dat_get_step_marks(dat_handle* h, double* marks_ms, int max_marks) {
  if (!h) return fail("null handle");
  const int m = (int)h->marks.size();
  if (marks_ms)
    for (int k = 0; k < m && k < max_marks; ++k) marks_ms[k] = h->marks[k] - h->marks[0];
  return m;
}

int dat_get_counters(dat_handle* h, long long* qp_solves, long long* ipm_iters, long long* ipm_row_iters,
                     long long* hl_steps, double* hl_kernel_ms) {
  if (!h) return fail("null handle");
  unsigned long long cc[DAT_NCOUNTERS];
  if (read_words(h, h->counters, cc, DAT_NCOUNTERS)) return -1;
  unsigned long long c[3] = {cc[0], cc[1], cc[2]};
  if (h->cfg.mode == DAT_MODE_CADMM)
    for (int k = 1; k < NCLS; ++k)
      for (int j = 0; j < 3; ++j) c[j] += cc[CNT_STRIDE * k + j];
  if (qp_solves) *qp_solves = (long long)c[0];
  if (ipm_iters) *ipm_iters = (long long)c[1];
  if (ipm_row_iters) *ipm_row_iters = (long long)c[2];
  if (hl_steps) *hl_steps = h->hl_steps;
  if (hl_kernel_ms) *hl_kernel_ms = h->hl_ms;
  return 0;
}

int dat_get_class_counters(dat_handle* h, int env_class, long long* qp_solves, long long* ipm_iters,
                           long long* ipm_row_iters, double* kernel_ms) {
  if (!h) return fail("null handle");
  if (h->cfg.mode != DAT_MODE_CADMM) return fail("dat_get_class_counters: C-ADMM handles only");
  if (env_class < 0 || env_class >= NCLS) return fail("dat_get_class_counters: env_class must be in [0, 4)");
  if (kernel_ms) *kernel_ms = h->cadmm_ms;
  return read_words(h, h->counters + CNT_STRIDE * env_class, {qp_solves, ipm_iters, ipm_row_iters});
}

int dat_get_class_occupancy(dat_handle* h, int env_class, long long* slot_ipm_iters, long long* wave_admm_iters) {
  if (!h) return fail("null handle");
  if (h->cfg.mode != DAT_MODE_CADMM) return fail("dat_get_class_occupancy: C-ADMM handles only");
  if (env_class < 0 || env_class >= NCLS) return fail("dat_get_class_occupancy: env_class must be in [0, 4)");
  return read_words(h, h->counters + CNT_STRIDE * env_class + 3, {slot_ipm_iters, wave_admm_iters});
}

int dat_reset_counters(dat_handle* h) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemsetAsync(h->counters, 0, DAT_NCOUNTERS * sizeof(unsigned long long), h->stream));
  {  // the running minimum of the env distance starts at +inf
    static const unsigned long long inf = dist_key(HUGE_VAL);
    HIPCHK(hipMemcpyAsync(h->counters + CNT_COLL + 1, &inf, sizeof(inf), hipMemcpyHostToDevice, h->stream));
  }
  if (h->advcnt) HIPCHK(hipMemsetAsync(h->advcnt, 0, 2 * sizeof(unsigned long long), h->stream));
  h->cadmm_ms = 0.0;
  HIPCHK(hipStreamSynchronize(h->stream));
  h->hl_steps = 0;
  h->hl_ms = 0.0;
  return 0;
}

int dat_set_sub_batches(dat_handle* h, int count) {
  if (!h) return fail("null handle");
  if (count < 1 || count > DAT_MAX_SUB) return fail("dat_set_sub_batches: count must be in [1, 4]");
  if (count > 1 && h->cfg.mode != DAT_MODE_CADMM) return fail("dat_set_sub_batches: C-ADMM handles only");
  if (count > h->cfg.batch) return fail("dat_set_sub_batches: more sub-batches than scenarios");
  if (count > 1 && h->cfg.record_err) return fail("dat_set_sub_batches: record_err must be 0");
  HIPCHK(hipSetDevice(h->cfg.device));
  // a handle keeps at most four streams: its own and the sub-batches' further ones, or (one sub-batch) its own and
  // on first use the tail's, the advance stream and the pipeline's second
  if (count > 1)
    for (side_stream* s : {&h->tail, &h->advance, &h->pipe}) side_release(h, s);
  for (int s = count; s < DAT_MAX_SUB; ++s)
    if (s > 0) side_release(h, &h->sub[s]);
  for (int s = 1; s < count; ++s) HIPCHK(side_get(h, &h->sub[s], 1));
  if (count > 1) {
    HIPCHK(own_event(h, &h->ev_start));
    HIPCHK(own_event(h, &h->ev_end));
  }
  h->nsub = count;
  return 0;
}

int dat_set_advance_overlap(dat_handle* h, int on) {
  if (!h) return fail("null handle");
  h->adv_on = on != 0;
  return 0;
}

int dat_set_step_pipeline(dat_handle* h, int on) {
  if (!h) return fail("null handle");
  h->pipe_on = on != 0;
  return 0;
}

int dat_set_fused_advance(dat_handle* h, int on) {
  if (!h) return fail("null handle");
  h->fused_on = on != 0;
  return 0;
}

int dat_get_fused_launches(dat_handle* h, long long* advance, long long* scatter) {
  if (!h) return fail("null handle");
  if (advance) *advance = h->n_advance;
  if (scatter) *scatter = h->n_scatter;
  return 0;
}

int dat_get_stream_count(dat_handle* h) {
  if (!h) return fail("null handle");
  return (int)h->streams.size();
}

int dat_get_advance_counts(dat_handle* h, long long* early, long long* late) {
  if (!h) return fail("null handle");
  return read_words(h, h->advcnt, {early, late});
}

int dat_debug_advance_split(dat_handle* h, const unsigned char* early_mask) {
  if (!h) return fail("null handle");
  if (h->cfg.mode != DAT_MODE_CADMM) return fail("dat_debug_advance_split: C-ADMM handles only");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!early_mask) {
    dfree(h, h->advmask);
    h->advmask = nullptr;
    return 0;
  }
  if (!h->advmask && dalloc(h, &h->advmask, (size_t)h->cfg.batch)) return -1;
  HIPCHK(hipMemcpyAsync(h->advmask, early_mask, (size_t)h->cfg.batch, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_debug_get_env_class(dat_handle* h, double* lhs, double* rhs, int* nrow, int* env_class) {
  if (!h || !lhs || !rhs || !nrow || !env_class) return fail("dat_debug_get_env_class: null argument");
  if (h->cfg.mode != DAT_MODE_CADMM) return fail("dat_debug_get_env_class: C-ADMM handles only");
  if (h->env_sub < 1) return fail("dat_debug_get_env_class: no control step has run");
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t st : h->streams) HIPCHK(hipStreamSynchronize(st));  // (the handle's own among them)
  const size_t B = h->cfg.batch, n = h->cfg.n, per = extent_of(h, &h->erows);
  std::vector<double> img(B * per);
  std::vector<unsigned> mask(B * extent_of(h, &h->emask));
  std::vector<int> need(B);
  HIPCHK(hipMemcpy(img.data(), h->erows, sizeof(double) * img.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(mask.data(), h->emask, sizeof(unsigned) * mask.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(need.data(), h->need, sizeof(int) * need.size(), hipMemcpyDeviceToHost));
  std::fill(lhs, lhs + B * n * DAT_NENV * 3, 0.0);
  std::fill(rhs, rhs + B * n * DAT_NENV, 0.0);
  const int S = h->env_sub;
  for (int s = 0; s < S; ++s) {  // the sub-batch's block of the image (sub_kargs): stride count n
    const SubRange r = sub_range(h->cfg.batch, s, S);
    const size_t off = (size_t)r.off, NA = (size_t)r.count * n;
    const double* blk = img.data() + per * off;
    for (size_t g = 0; g < NA; ++g) {
      const size_t t = off * n + g;  // scenario-major index of the agent in the whole batch
      const unsigned m = mask[t];
      int k = 0;
      for (int j = 0; j < DAT_NENV; ++j) {
        if (!((m >> j) & 1u)) continue;
        for (int c = 0; c < 3; ++c) lhs[(t * DAT_NENV + k) * 3 + c] = blk[(4 * j + c) * NA + g];
        rhs[t * DAT_NENV + k] = blk[(4 * j + 3) * NA + g];
        ++k;
      }
      nrow[t] = k;
    }
  }
  for (size_t sc = 0; sc < B; ++sc) env_class[sc] = need[sc] >= NKEY ? need[sc] - NKEY : need[sc] / NIB;
  return 0;
}

int dat_set_persistent_blocks(dat_handle* h, int blocks) {
  if (!h) return fail("null handle");
  if (blocks < 0) return fail("dat_set_persistent_blocks: negative");
  if (blocks == 0) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->cfg.device) != hipSuccess || ncu <= 0)
      ncu = 256;
    blocks = 4 * ncu;
  }
  h->persistent_blocks = blocks;
  return 0;
}

int dat_cadmm_slots(dat_handle* h, int batch, int* slots) {
  if (!h) return fail("null handle");
  if (h->cfg.mode != DAT_MODE_CADMM) return fail("dat_cadmm_slots: C-ADMM handles only");
  if (batch < 1 || !slots) return fail("dat_cadmm_slots: batch must be positive and slots non-null");
  *slots = cadmm_slots(h, batch, h->cfg.n);
  return 0;
}

int dat_cadmm_row_mode(int n, int slots, int env_class) {
  if (n < 1 || n > 64 || slots < 1 || slots > 64 / n || env_class < 0 || env_class >= NCLS) return -1;
  return cadmm_row_mode(n, slots, env_class);
}

int dat_synchronize(dat_handle* h) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_env_rows(dat_handle* h, double* lhs, double* rhs, int* nrow, unsigned char* collision, double* min_dist) {
  if (!h || !lhs || !rhs || !nrow || !collision || !min_dist) return fail("dat_env_rows: null argument");
  if (!h->have_params) return fail("dat_env_rows: params not set");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = h->cfg.batch, n = h->cfg.n, T = B * n;
  Scratch tmp;
  double *dl = tmp.get<double>(T * DAT_NENV * 3), *dr = tmp.get<double>(T * DAT_NENV), *dm = tmp.get<double>(T);
  int* dn = tmp.get<int>(T);
  unsigned char* dc = tmp.get<unsigned char>(T);
  if (!dl || !dr || !dm || !dn || !dc) return fail("dat_env_rows: device allocation failed");
  KArgs a = kargs(h);
  hipLaunchKernelGGL(k_env, dim3((T + 63) / 64), dim3(64), 0, h->stream, a, dl, dr, dn, dc, dm);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(lhs, dl, sizeof(double) * T * DAT_NENV * 3, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(rhs, dr, sizeof(double) * T * DAT_NENV, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(nrow, dn, sizeof(int) * T, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(collision, dc, T, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(min_dist, dm, sizeof(double) * T, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

namespace {
// dat_solve_agent_qp_batch (env_lhs = null: the forest query) and dat_solve_agent_qp_rows_batch (the caller's rows)
int solve_agent_qp_batch(const char* who, dat_handle* h, int count, const int* scenario, const int* agent,
                         const double* acc_des, const double* lam, const double* rho, const double* f_mean,
                         const double* c9, const double* env_lhs, const double* env_rhs, const int* nenv, double* x,
                         int* status, int* ipm_iters, unsigned char* collision, double* min_env_dist,
                         unsigned char* certified) {
  const std::string W = std::string(who) + ": ";
  if (!h) return fail("null handle");
  if (count < 0) return fail(W + "negative count");
  if (count == 0) return 0;
  if (!h->have_params) return fail(W + "params not set");
  const int mode = h->cfg.mode, n = h->cfg.n, N3 = 3 * n;
  if (mode == DAT_MODE_CENTRALIZED) return fail(W + "C-ADMM or DD handles only");
  const bool dd = mode == DAT_MODE_DD;
  if (!scenario || !agent || !acc_des || !x || !status) return fail(W + "null argument");
  if (dd ? !c9 : (!lam || !rho || !f_mean)) return fail(W + "missing multipliers");
  if (env_lhs && (!env_rhs || !nenv)) return fail(W + "null argument");
  for (int k = 0; k < count; ++k) {
    if (env_lhs && (nenv[k] < 0 || nenv[k] > DAT_NENV)) return fail(W + "nenv out of range");
    if (scenario[k] < 0 || scenario[k] >= h->cfg.batch) return fail(W + "scenario out of range");
    if (agent[k] < 0 || agent[k] >= n) return fail(W + "agent out of range");
    if (!dd && !(rho[k] > 0.0))
      return fail(W + "rho must be > 0 (at rho = 0 the copies f_j, j != i, are not unique)");
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t C = count, nx = dd ? 9 : N3;
  Scratch tmp;
  bool ok = true;
  auto dev = [&](size_t bytes, const void* src) -> void* {
    void* p = tmp.get<char>(bytes);
    ok = ok && p && (!src || hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, h->stream) == hipSuccess);
    return p;
  };
  AgentQPArgs q;
  memset(&q, 0, sizeof(q));
  q.count = count;
  q.scen = (const int*)dev(sizeof(int) * C, scenario);
  q.agent = (const int*)dev(sizeof(int) * C, agent);
  q.acc = (const double*)dev(sizeof(double) * C * 6, acc_des);
  if (dd) {
    q.c9 = (const double*)dev(sizeof(double) * C * 9, c9);
  } else {
    q.lam = (const double*)dev(sizeof(double) * C * N3, lam);
    q.rho = (const double*)dev(sizeof(double) * C, rho);
    q.fbar = (const double*)dev(sizeof(double) * C * N3, f_mean);
  }
  if (env_lhs) {
    q.elhs = (const double*)dev(sizeof(double) * C * DAT_NENV * 3, env_lhs);
    q.erhs = (const double*)dev(sizeof(double) * C * DAT_NENV, env_rhs);
    q.nenv = (const int*)dev(sizeof(int) * C, nenv);
  }
  q.x = (double*)dev(sizeof(double) * C * nx, nullptr);
  q.status = (int*)dev(sizeof(int) * C, nullptr);
  q.iters = (int*)dev(sizeof(int) * C, nullptr);
  q.col = (unsigned char*)dev(C, nullptr);
  q.mind = (double*)dev(sizeof(double) * C, nullptr);
  q.best = (double*)dev(sizeof(double) * C * best_size(1), nullptr);
  q.cert = (unsigned char*)dev(C, nullptr);
  if (!ok) return fail(W + "device allocation failed");
  KArgs a = kargs(h);
  HIPCHK(hipEventRecord(h->e0, h->stream));
  hipLaunchKernelGGL(k_agent_qp, dim3((count + 63) / 64), dim3(64), 0, h->stream, a, q);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->e1, h->stream));
  HIPCHK(hipMemcpyAsync(x, q.x, sizeof(double) * C * nx, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(status, q.status, sizeof(int) * C, hipMemcpyDeviceToHost, h->stream));
  if (ipm_iters) HIPCHK(hipMemcpyAsync(ipm_iters, q.iters, sizeof(int) * C, hipMemcpyDeviceToHost, h->stream));
  if (collision) HIPCHK(hipMemcpyAsync(collision, q.col, C, hipMemcpyDeviceToHost, h->stream));
  if (min_env_dist) HIPCHK(hipMemcpyAsync(min_env_dist, q.mind, sizeof(double) * C, hipMemcpyDeviceToHost, h->stream));
  if (certified) HIPCHK(hipMemcpyAsync(certified, q.cert, C, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->e0, h->e1) == hipSuccess) h->agent_qp_ms = ms;
  return 0;
}
}  // namespace

int dat_solve_agent_qp_batch(dat_handle* h, int count, const int* scenario, const int* agent, const double* acc_des,
                             const double* lam, const double* rho, const double* f_mean, const double* c9, double* x,
                             int* status, int* ipm_iters, unsigned char* collision, double* min_env_dist) {
  return solve_agent_qp_batch("dat_solve_agent_qp_batch", h, count, scenario, agent, acc_des, lam, rho, f_mean, c9,
                              nullptr, nullptr, nullptr, x, status, ipm_iters, collision, min_env_dist, nullptr);
}

int dat_solve_agent_qp_rows_batch(dat_handle* h, int count, const int* scenario, const int* agent,
                                  const double* acc_des, const double* lam, const double* rho, const double* f_mean,
                                  const double* c9, const double* env_lhs, const double* env_rhs, const int* nenv,
                                  double* x, int* status, int* ipm_iters, unsigned char* collision,
                                  double* min_env_dist, unsigned char* certified) {
  if (!env_lhs || !env_rhs || !nenv) return fail("dat_solve_agent_qp_rows_batch: null argument");
  return solve_agent_qp_batch("dat_solve_agent_qp_rows_batch", h, count, scenario, agent, acc_des, lam, rho, f_mean,
                              c9, env_lhs, env_rhs, nenv, x, status, ipm_iters, collision, min_env_dist, certified);
}

int dat_set_low_level(dat_handle* h, int kind) {
  if (!h) return fail("null handle");
  if (kind != DAT_LL_PD && kind != DAT_LL_SM) return fail("dat_set_low_level: kind must be DAT_LL_PD or DAT_LL_SM");
  h->ll_kind = kind;
  return 0;
}

int dat_low_level_control(dat_handle* h, const double* f_des, double* thrust, double* moment) {
  if (!h || !thrust || !moment) return fail("dat_low_level_control: null argument");
  if (!h->have_params) return fail("dat_low_level_control: params not set");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = h->cfg.batch, n = h->cfg.n;
  if (f_des) HIPCHK(hipMemcpyAsync(h->fdes, f_des, sizeof(double) * B * 3 * n, hipMemcpyHostToDevice, h->stream));
  Scratch tmp;
  double *df = tmp.get<double>(B * n), *dm = tmp.get<double>(B * n * 3);
  if (!df || !dm) return fail("dat_low_level_control: device allocation failed");
  KArgs a = kargs(h);
  hipLaunchKernelGGL(k_low_level, dim3((B * n + 63) / 64), dim3(64), 0, h->stream, a, (const double*)h->fdes, df, dm);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(thrust, df, sizeof(double) * B * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(moment, dm, sizeof(double) * B * n * 3, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_get_kernel_ms(dat_handle* h, double* ms) {
  if (!h || !ms) return fail("dat_get_kernel_ms: null argument");
  *ms = h->cadmm_ms;
  return 0;
}

int dat_get_agent_qp_ms(dat_handle* h, double* ms) {
  if (!h || !ms) return fail("dat_get_agent_qp_ms: null argument");
  *ms = h->agent_qp_ms;
  return 0;
}

int dat_get_robust_redos(dat_handle* h, long long* redos) {
  if (!h) return fail("dat_get_robust_redos: null handle");
  return read_words(h, h->counters + CNT_ROB, {redos});
}

int dat_get_tail_counters(dat_handle* h, long long* out) {
  if (!h || !out) return fail("dat_get_tail_counters: null argument");
  return read_words(h, h->counters + CNT_TAIL, {out, out + 1, out + 2, out + 3, out + 4, out + 5});
}

int dat_get_collision_stats(dat_handle* h, long long* collisions, double* min_env_dist) {
  if (!h) return fail("dat_get_collision_stats: null handle");
  unsigned long long c[2];
  if (read_words(h, h->counters + CNT_COLL, c, 2)) return -1;
  if (collisions) *collisions = (long long)c[0];
  if (min_env_dist) *min_env_dist = dist_of_key(c[1]);
  return 0;
}

int dat_get_inband_exits(dat_handle* h, long long* inband, long long* beyond_clarabel_tol) {
  if (!h) return fail("dat_get_inband_exits: null handle");
  return read_words(h, h->counters + CNT_INBAND, {inband, beyond_clarabel_tol});
}

int dat_rp_rollout(dat_handle* h, int steps, const double* f) {
  if (!h) return fail("null handle");
  if (steps <= 0) return 0;
  if (!h->have_params) return fail("dat_rp_rollout: params not set");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = h->cfg.batch, n = h->cfg.n;
  if (f) HIPCHK(hipMemcpyAsync(h->fdes, f, sizeof(double) * B * 3 * n, hipMemcpyHostToDevice, h->stream));
  KArgs a = kargs(h);
  hipLaunchKernelGGL(k_rp_rollout, dim3((B + 63) / 64), dim3(64), 0, h->stream, a, steps, h->cfg.dt,
                     (const double*)h->fdes);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

namespace {
// the handle's buffer of the PMRL entry points, at least `need` doubles
int pmrl_reserve(dat_handle* h, size_t need) {
  if (need <= h->pmrl_cap) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  dfree(h, h->pmrl_buf);
  h->pmrl_cap = 0;
  if (dalloc(h, &h->pmrl_buf, need)) return -1;
  h->pmrl_cap = need;
  return 0;
}
}  // namespace

int dat_pmrl_rollout(dat_handle* h, int steps, const double* f, int nf) {
  if (!h) return fail("dat_pmrl_rollout: null handle");
  if (!f) return fail("dat_pmrl_rollout: null force schedule");
  if (steps < 0) return fail("dat_pmrl_rollout: negative steps");
  if (nf < 1) return fail("dat_pmrl_rollout: nf must be >= 1");
  if (steps % nf != 0)
    return fail("dat_pmrl_rollout: steps (" + std::to_string(steps) + ") must be a multiple of nf (" +
                std::to_string(nf) + ")");
  if (!h->have_params) return fail("dat_pmrl_rollout: params not set");
  if (steps == 0) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  const int B = h->cfg.batch, n = h->cfg.n;
  const size_t words = (size_t)nf * B * 3 * n;
  if (pmrl_reserve(h, words)) return -1;
  HIPCHK(hipMemcpyAsync(h->pmrl_buf, f, sizeof(double) * words, hipMemcpyHostToDevice, h->stream));
  KArgs a = kargs(h);
  const int G = 64 / n;
  hipLaunchKernelGGL(k_pmrl_rollout, dim3((B + G - 1) / G), dim3(64), 0, h->stream, a, steps, nf, h->cfg.dt,
                     (const double*)h->pmrl_buf);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_pmrl_forward(dat_handle* h, const double* f, double* ddq, double* dvl, double* dwl, double* T) {
  if (!h) return fail("dat_pmrl_forward: null handle");
  if (!f || !ddq || !dvl || !dwl || !T) return fail("dat_pmrl_forward: null argument");
  if (!h->have_params) return fail("dat_pmrl_forward: params not set");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int B = h->cfg.batch, n = h->cfg.n;
  // f, ddq (3n each), T (n), dvl, dwl (3 each) per scenario, one after the other
  const size_t of = 0, oq = (size_t)B * 3 * n, oT = 2 * oq, ov = oT + (size_t)B * n, ow = ov + (size_t)B * 3;
  if (pmrl_reserve(h, ow + (size_t)B * 3)) return -1;
  double* d = h->pmrl_buf;
  HIPCHK(hipMemcpyAsync(d + of, f, sizeof(double) * oq, hipMemcpyHostToDevice, h->stream));
  KArgs a = kargs(h);
  const int G = 64 / n;
  hipLaunchKernelGGL(k_pmrl_forward, dim3((B + G - 1) / G), dim3(64), 0, h->stream, a, (const double*)(d + of), d + oq,
                     d + ov, d + ow, d + oT);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ddq, d + oq, sizeof(double) * oq, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(T, d + oT, sizeof(double) * B * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(dvl, d + ov, sizeof(double) * B * 3, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(dwl, d + ow, sizeof(double) * B * 3, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- the closed loop's log --------------------------------------------------------------------------------
int dat_log_begin(dat_handle* h, const int* scenarios, int count, int log_every, int hl_capacity, int summary) {
  if (!h) return fail("null handle");
  if (h->log.open) return fail("dat_log_begin: a log is already open (dat_log_end first)");
  const int B = h->cfg.batch, n = h->cfg.n;
  if (count < 0 || count > B) return fail("dat_log_begin: count must be in [0, batch]");
  if (!scenarios && count != 0 && count != B)
    return fail("dat_log_begin: scenarios = NULL needs count = 0 (none) or count = batch (all)");
  if (log_every < 1) return fail("dat_log_begin: log_every must be >= 1");
  if (hl_capacity < 1) return fail("dat_log_begin: hl_capacity must be >= 1");
  std::vector<int> map((size_t)B, -1);
  for (int k = 0; k < count; ++k) {
    const int sc = scenarios ? scenarios[k] : k;
    if (sc < 0 || sc >= B || (k > 0 && scenarios && sc <= scenarios[k - 1]))
      return fail("dat_log_begin: scenarios must be strictly increasing indices in [0, batch)");
    map[sc] = k;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  dat_log& g = h->log;
  g.nslot = count;
  g.log_every = log_every;
  g.hl_cap = hl_capacity;
  // the logged steps of hl_capacity HL periods, whatever the clock's phase against log_every
  g.step_cap = ((long long)hl_capacity * h->cfg.hl_every + log_every - 1) / log_every + 1;
  const size_t rows = (size_t)hl_capacity * B;
  hipError_t e = hipMalloc((void**)&g.slot, sizeof(int) * (size_t)B);
  if (e == hipSuccess && count > 0)
    e = hipMalloc((void**)&g.hl, sizeof(double) * (size_t)hl_capacity * count * DAT_LOG_HL_WORDS(n));
  if (e == hipSuccess && count > 0)
    e = hipMalloc((void**)&g.step, sizeof(double) * (size_t)g.step_cap * count * DAT_LOG_ST_WORDS(n));
  if (e == hipSuccess && summary) e = hipMalloc((void**)&g.sum_iters, sizeof(int) * rows);
  if (e == hipSuccess && summary) e = hipMalloc((void**)&g.sum_mind, sizeof(double) * rows);
  if (e == hipSuccess && summary) e = hipMalloc((void**)&g.sum_col, rows);
  if (e == hipSuccess) e = hipMemcpyAsync(g.slot, map.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    log_free(h);
    return fail(std::string("dat_log_begin: ") + hipGetErrorString(e));
  }
  g.open = true;
  return 0;
}

int dat_log_counts(dat_handle* h, long long* hl_records, long long* step_records, long long* clock) {
  if (!h) return fail("null handle");
  if (!h->log.open) return fail("dat_log_counts: no log open");
  if (hl_records) *hl_records = h->log.hl_count(h->cfg.hl_every);
  if (step_records) *step_records = h->log.step_count();
  if (clock) *clock = h->log.clock;
  return 0;
}

namespace {
// records [first, first + count) of a full-tier buffer, copied to the host
int log_fetch(dat_handle* h, const char* who, const double* buf, long long held, int first, int count, size_t words,
              std::vector<double>* out) {
  if (!h) return fail("null handle");
  if (!h->log.open) return fail(std::string(who) + ": no log open");
  if (first < 0 || count < 0 || (long long)first + count > held)
    return fail(std::string(who) + ": records [first, first + count) must lie in the " + std::to_string(held) + " held");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t rec = (size_t)h->log.nslot * words;
  out->resize((size_t)count * rec);
  if (out->empty()) return 0;
  HIPCHK(hipMemcpyAsync(out->data(), buf + (size_t)first * rec, sizeof(double) * out->size(), hipMemcpyDeviceToHost,
                        h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
}  // namespace

int dat_log_read_hl(dat_handle* h, int first, int count, double* f_des, int* iters, int* qp_status, double* min_env_dist,
                    unsigned char* collision, double* x_ref, double* v_ref, double* solve_ms) {
  std::vector<double> w;
  if (log_fetch(h, "dat_log_read_hl", h ? h->log.hl : nullptr, h && h->log.open ? h->log.hl_count(h->cfg.hl_every) : 0,
                first, count, DAT_LOG_HL_WORDS(h ? h->cfg.n : 3), &w))
    return -1;
  const size_t n = h->cfg.n, R = h->log.nslot, HW = DAT_LOG_HL_WORDS(n);
  for (size_t k = 0; k < (size_t)count * R; ++k) {
    const double* r = w.data() + k * HW;
    int ri[2 + NMAX];
    memcpy(ri, r + DAT_LOG_HL_INTS(n), sizeof(int) * (2 + n));
    if (f_des) memcpy(f_des + k * 3 * n, r, sizeof(double) * 3 * n);
    if (iters) iters[k] = ri[0];
    if (collision) collision[k] = (unsigned char)ri[1];
    if (qp_status) memcpy(qp_status + k * n, ri + 2, sizeof(int) * n);
    if (min_env_dist) min_env_dist[k] = r[DAT_LOG_HL_MIND(n)];
    if (x_ref) memcpy(x_ref + 3 * k, r + DAT_LOG_HL_XREF(n), sizeof(double) * 3);
    if (v_ref) memcpy(v_ref + 3 * k, r + DAT_LOG_HL_VREF(n), sizeof(double) * 3);
  }
  if (solve_ms)
    for (int k = 0; k < count; ++k) solve_ms[k] = h->log.hl_ms[(size_t)first + k];
  return 0;
}

int dat_log_read_steps(dat_handle* h, int first, int count, long long* step_index, double* thrust, double* moment,
                       double* state, double* x_err, double* v_err) {
  std::vector<double> w;
  if (log_fetch(h, "dat_log_read_steps", h ? h->log.step : nullptr, h && h->log.open ? h->log.step_count() : 0, first,
                count, DAT_LOG_ST_WORDS(h ? h->cfg.n : 3), &w))
    return -1;
  const size_t n = h->cfg.n, R = h->log.nslot, SW = DAT_LOG_ST_WORDS(n), S = DAT_STATE_SIZE(n);
  for (size_t k = 0; k < (size_t)count * R; ++k) {
    const double* r = w.data() + k * SW;
    for (size_t i = 0; i < n; ++i) {
      if (thrust) thrust[k * n + i] = r[4 * i];
      if (moment) memcpy(moment + (k * n + i) * 3, r + 4 * i + 1, sizeof(double) * 3);
    }
    if (state) memcpy(state + k * S, r + DAT_LOG_ST_STATE(n), sizeof(double) * S);
    if (x_err) x_err[k] = r[DAT_LOG_ST_XERR(n)];
    if (v_err) v_err[k] = r[DAT_LOG_ST_XERR(n) + 1];
  }
  if (step_index)
    for (int k = 0; k < count; ++k) step_index[k] = (h->log.step_base + first + k) * h->log.log_every;
  return 0;
}

int dat_log_read_summary(dat_handle* h, int first, int count, int* iters, double* min_env_dist,
                         unsigned char* collision) {
  if (!h) return fail("null handle");
  const dat_log& g = h->log;
  if (!g.open || !g.sum_iters) return fail("dat_log_read_summary: no log with the summary tier open");
  const long long held = g.hl_count(h->cfg.hl_every);
  if (first < 0 || count < 0 || (long long)first + count > held)
    return fail("dat_log_read_summary: records [first, first + count) must lie in the " + std::to_string(held) + " held");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = h->cfg.batch, o = (size_t)first * B, m = (size_t)count * B;
  if (m == 0) return 0;
  if (iters) HIPCHK(hipMemcpyAsync(iters, g.sum_iters + o, sizeof(int) * m, hipMemcpyDeviceToHost, h->stream));
  if (min_env_dist)
    HIPCHK(hipMemcpyAsync(min_env_dist, g.sum_mind + o, sizeof(double) * m, hipMemcpyDeviceToHost, h->stream));
  if (collision) HIPCHK(hipMemcpyAsync(collision, g.sum_col + o, m, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_log_clear(dat_handle* h) {
  if (!h) return fail("null handle");
  dat_log& g = h->log;
  if (!g.open) return fail("dat_log_clear: no log open");
  g.hl_base = g.clock / h->cfg.hl_every;
  g.step_base = (g.clock + g.log_every - 1) / g.log_every;
  g.hl_ms.clear();
  return 0;
}

int dat_log_end(dat_handle* h) {
  if (!h) return fail("null handle");
  if (!h->log.open) return fail("dat_log_end: no log open");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  log_free(h);
  return 0;
}

}  // extern "C"
