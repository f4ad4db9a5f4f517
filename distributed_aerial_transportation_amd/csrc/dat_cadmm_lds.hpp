// dat_cadmm_lds.hpp -- the LDS arithmetic of the C-ADMM drain, stated once for the kernels that carve by it
// (dat_cadmm_drain.hpp) and the host that sizes their launches by it (dat.hip).
#pragma once

#include "dat_drain_common.hpp"

// Internal linkage, as in the one unit this text came from: each unit's inliner weighs these functions as it did
// there, and a kernel keeps its symbol.
namespace {
using namespace dat;

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
// per-slot ints done / sid / wmx (G each), rounded to 16 bytes
__host__ __device__ constexpr int slot_ints(int G) { return (3 * G + 3) & ~3; }
__host__ __device__ constexpr size_t cadmm_fixed_bytes(int n, int G) {
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
__host__ __device__ constexpr size_t cadmm_area_doubles(int cls, int rmode) {
  const size_t rows = rmode ? (size_t)row_lds_doubles(cadmm_nr(cls), cadmm_aux_doubles(cls, rmode)) : 0;
  return (rows > 64 * RDS ? rows : 64 * RDS) + (size_t)env_lds_doubles(class_env_rows(cls));
}
// row state of class cls in LDS: with the class's aux slots when that carve fits the budget, else rows
// alone for classes ROWLDS_MIN_CLS .. 2; class 3 (13 slots) never.  Few row slots without aux slots
// are cheaper in registers: an LDS row access costs an LDS round trip, which pays only once the rows
// would otherwise spill.
constexpr int ROWLDS_MIN_CLS = 1;
__host__ __device__ constexpr int cadmm_row_mode(int n, int G, int cls) {
  if (cls >= NCLS - 1) return 0;
  if (cadmm_auxm(cls) && cadmm_fixed_bytes(n, G) + sizeof(double) * cadmm_area_doubles(cls, 2) <= LDS_WAVE_BUDGET)
    return 2;
  if (cls >= ROWLDS_MIN_CLS && cadmm_fixed_bytes(n, G) + sizeof(double) * cadmm_area_doubles(cls, 1) <= LDS_WAVE_BUDGET)
    return 1;
  return 0;
}
// The row modes of a launch, classes 0 .. 2 in two bits each (class 3: always registers).  The mode is a template
// parameter of the drain (cadmm_drain<CLS, ., ., RMODE>: each class drain carries the one IPM instantiation it runs),
// so a launch picks the k_cadmm / k_cadmm0 instantiation of its word: cadmm_row_modes(n, G), the rule above, which
// sizes the carve too -- kernel and carve go by the same word (launch_cadmm, dat.hip).
__host__ __device__ constexpr int rm_pack(int m0, int m1, int m2) { return m0 | (m1 << 2) | (m2 << 4); }
__host__ __device__ constexpr int rm_of(int rms, int cls) { return cls >= NCLS - 1 ? 0 : (rms >> (2 * cls)) & 3; }
__host__ __device__ constexpr int cadmm_row_modes(int n, int G) {
  return rm_pack(cadmm_row_mode(n, G, 0), cadmm_row_mode(n, G, 1), cadmm_row_mode(n, G, 2));
}
// The words the kernel units instantiate (DAT_CADMM_RMS: one line per word, in launchers and here): every word the
// rule gives for 3 <= n <= NMAX and 1 <= G <= 64 / n.  Classes 0 and 1 always fit with their aux slots; class 2
// loses them where the fixed part is large (n = 3 .. 5 at the largest G).
#define DAT_CADMM_RMS(X) X(2, 2, 2) X(2, 2, 1)
__host__ __device__ constexpr bool cadmm_rms_built(int rms) {
#define DAT_X(m0, m1, m2) if (rms == rm_pack(m0, m1, m2)) return true;
  DAT_CADMM_RMS(DAT_X)
#undef DAT_X
  return false;
}
__host__ __device__ constexpr bool cadmm_rms_cover(int nmax) {
  for (int n = 3; n <= nmax; ++n)
    for (int G = 1; G <= 64 / n; ++G)
      if (!cadmm_rms_built(cadmm_row_modes(n, G))) return false;
  return true;
}
static_assert(cadmm_rms_cover(NMAX), "cadmm_row_mode gives a word DAT_CADMM_RMS does not list");
// dynamic LDS of a k_cadmm workgroup: the largest carve of the env classes that can occur (without a
// forest every scenario is class 0, so the launch needs only that carve and more workgroups fit a CU), by the
// launch's row modes
__host__ __device__ constexpr size_t cadmm_lds_bytes_of(int n, int G, int max_cls, int rms) {
  size_t m = 0;
  for (int c = 0; c <= max_cls; ++c) {
    const size_t b = cadmm_fixed_bytes(n, G) + sizeof(double) * cadmm_area_doubles(c, rm_of(rms, c));
    m = b > m ? b : m;
  }
  return m;
}
__host__ __device__ constexpr size_t cadmm_lds_bytes(int n, int G, int max_cls = NCLS - 1) {
  return cadmm_lds_bytes_of(n, G, max_cls, cadmm_row_modes(n, G));
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

}  // namespace
