// dat_launch.hpp -- the seam between dat.hip (handle, step chain, C-ABI: host code only) and the kernel units
// beside it, one per kernel family, which compile in parallel:
//   dat_k_cadmm.hip       k_cadmm<false, .>, k_cadmm0<false, .> (one per row-mode word, DAT_CADMM_RMS); k_dd<false>
//   dat_k_cadmm_adv.hip   k_cadmm<true, .>, k_cadmm0<true, .> (the closed loop's advance overlap); k_dd<true>
//   dat_k_cadmm_tail.hip  k_cadmm_tail, k_cadmm0_tail, the raise of their dynamic-LDS limit; k_agent_qp
//   dat_k_dd.hip          k_dd_setup<0, 3..8>, k_dd_key, the byte counts of the DD carves
//   dat_k_step.hip        the rollout / advance family as a whole (the inliner's choices for the device functions it
//                         shares depend on the callers the unit holds), the sorts, k_warm, k_env, the rigid-payload,
//                         PMRL and checkpoint kernels
// Why the kernels that solve agent QPs are grouped so: the split placed them so that every unit calling the
// out-of-line build_shared (dat_qp.hpp) held callers that pass it different constants (cadmm = true from the C-ADMM
// drains, false from k_dd), which kept the compiler from specialising it per unit.  The C-ADMM drains build inline
// now (build_shared_inl, one site: the drain kernels hold no call), so the out-of-line function's callers are k_dd in
// the two drain units, where it is specialised for cadmm = false, and k_agent_qp in the tail unit, which passes a
// run-time value: the function differs between the units (tools/same_kernels.py reports it SPLIT) and k_dd's
// register allocation follows its version.  The arithmetic is the text's in each: -ffp-contract=on fuses within
// an expression only.  The grouping stays for the balance of the units' compile times (profiles/tu_split.md).
// Each unit exports thin launchers, as dat_cent.hip does (launch_cent, dat_kargs.hpp): one kernel launch each, on the
// caller's grid, LDS bytes and stream, the instantiation picked by the selectors (adv, forest, env, n); they hold
// no state, know nothing of the handle and return the launch's error (hipGetLastError).  Every sequence of
// launches, events and streams is dat.hip's.
//
// The development builds' device globals (g_phase, g_iter_hist, g_cap) are written by several families and read by
// dat.hip, which one unit can hold without relocatable device code: those builds compile dat_unity.hip, all the
// units as one (tools/build_var.sh).
#pragma once

#include <cstring>

#include "dat_ckpt.hpp"
#include "dat_kargs.hpp"

#if (defined(DAT_PHASE_PROF) || defined(DAT_ITER_HIST) || defined(DAT_CAPTURE_LOOSE)) && !defined(DAT_UNITY)
#error "DAT_PHASE_PROF / DAT_ITER_HIST / DAT_CAPTURE_LOOSE builds share device globals between the kernel units: compile csrc/dat_unity.hip (tools/build_var.sh), not the units one by one"
#endif

// Internal linkage, as in the one unit this text came from.
namespace {

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

// the key tables of the filtered sorts (k_advance counts, k_bucket_scatter scatters: dat_k_step.hip)
constexpr int KT_COUNT = 0, KT_CURSOR = dat::NKEY_ALL, KT_INTS = 2 * dat::NKEY_ALL;  // KeyTab: counts, then scatter cursors

}  // namespace

namespace dat {

// The argument records the host fills for k_agent_qp and the checkpoint kernels.  (The kernels take them as types
// of their units' own, derived from these and named alike, so their symbols are what they were.)
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

// The open episodes (dat_episode_*), handed to the kernels with the episode flag (k_rollout_agents<., ., true>,
// k_advance<., true>) at every HL step: the rules, the pool, the outcome table and the record's segments in the
// handle's arrays, which a respawn writes (ck: the whole batch's arrays, indexed by off + the sub-batch's scenario).
enum EpCounter {
  EPC_COUNT,                           // outcomes appended or dropped since the last clear: the table's cursor
  EPC_LOST,                            // ... dropped, beyond the capacity
  EPC_IDLE,                            // idle slots
  EPC_ENDED,                           // [EPC_ENDED + reason] episodes ended per reason since dat_episode_begin
  EPC_RESPAWN = EPC_ENDED + DAT_EP_NREASON,  // respawns by [0] the early pass (never), [1] every other pass;
  EPC_DEFERRED = EPC_RESPAWN + 2,      // ending scenarios the early gate left to the rest pass
  EPC_WORDS
};
struct EpArgs {
  dat_episode_rules rules;
  const double* pool;  // P records of ck.words words
  int P;
  int batch, off;      // the handle's batch; the global index of the launch's scenario 0 (sub-batches)
  int hl_every;
  long long tick;      // the tick of the control step the launch follows
  double* table;       // cap outcome records of DAT_EP_WORDS words
  int cap;
  unsigned long long* cnt;  // EpCounter
  CkArgs ck;
};
struct NoEp {};

// ---- dat_k_cadmm.hip, dat_k_cadmm_adv.hip: forest ? k_cadmm<ADV, rms> : k_cadmm0<ADV, class 0's mode>, ADV the unit's;
// k_dd<false>, k_dd<true>
// rms: the launch's row modes (rm_pack, dat_cadmm_lds.hpp), the word `lds` was sized by: the instantiation of that word
// (hipErrorInvalidValue: the word is not built)
hipError_t launch_k_cadmm(bool forest, int rms, int blocks, size_t lds, hipStream_t st, const KArgs& a);
hipError_t launch_k_cadmm_adv(bool forest, int rms, int blocks, size_t lds, hipStream_t st, const KArgs& a);
hipError_t launch_k_dd(int blocks, size_t lds, hipStream_t st, const KArgs& a);
hipError_t launch_k_dd_env(int blocks, size_t lds, hipStream_t st, const KArgs& a);
// ---- dat_k_cadmm_tail.hip: forest ? k_cadmm_tail : k_cadmm0_tail; k_agent_qp
hipError_t launch_k_cadmm_tail(bool forest, int blocks, size_t lds, hipStream_t st, const KArgs& a);
hipError_t launch_k_agent_qp(hipStream_t st, const KArgs& a, const AgentQPArgs& q);
// the tail kernels' dynamic-LDS limit on `device` raised to a team of n's carve (dat_create; raise-only, per device)
hipError_t tail_lds_limit_raise(int device, int n);
// ---- dat_k_dd.hip
size_t dd_lds(int n, bool env);  // dynamic LDS of a k_dd / k_dd_setup workgroup: the byte counts of their carves
size_t dd_setup_lds(int n);
hipError_t launch_k_dd_setup(int blocks, size_t lds, hipStream_t st, const KArgs& a);  // k_dd_setup<n | 0> by a.n
hipError_t launch_k_dd_key(hipStream_t st, const KArgs& a);
// ---- dat_k_step.hip; adv: ADV_ALL / ADV_EARLY / ADV_REST (the sorts: ADV_ALL is k_bucket)
hipError_t launch_k_desired(int adv, hipStream_t st, const KArgs& a, double* acc);
hipError_t launch_k_env_class(int adv, int blocks, hipStream_t st, const KArgs& a);
hipError_t launch_k_bucket(hipStream_t st, int B, const int* need, int* list, int* count);
hipError_t launch_k_bucket_adv(int adv, hipStream_t st, int B, const int* need, int* list, int* count, const int* advp,
                               int serial);
hipError_t launch_k_bucket_scatter(int adv, hipStream_t st, int B, const int* need, int* list, int* count,
                                   const int* advp, int serial, int* tab, int* other);
// lg: the open log's arguments (k_rollout_agents<true, ADV_ALL>), or null; ep: the open episodes' (the instantiations
// with the episode flag; not with a log), or null: the kernels as they are without episodes
hipError_t launch_k_rollout_agents(const LogArgs* lg, int adv, int blocks, hipStream_t st, const KArgs& a, int steps,
                                   double dt, const double* fdes, const EpArgs* ep = nullptr);
hipError_t launch_k_advance(int adv, int blocks, hipStream_t st, const KArgs& a, int steps, double dt,
                            const double* fdes, double* acc, int* kc_lo, int* kc_hi, const EpArgs* ep = nullptr);
hipError_t launch_k_low_level(hipStream_t st, const KArgs& a, const double* fdes, double* fo, double* Mo);
hipError_t launch_k_rp_rollout(hipStream_t st, const KArgs& a, int steps, double dt, const double* f);
// acc: where the next step's desired acceleration goes (a.tick: that step's), or null: none
hipError_t launch_k_rp_advance(hipStream_t st, const KArgs& a, int steps, double dt, const double* f, double* acc);
hipError_t launch_k_pmrl_rollout(int blocks, hipStream_t st, const KArgs& a, int steps, int nf, double dt,
                                 const double* f);
hipError_t launch_k_pmrl_forward(int blocks, hipStream_t st, const KArgs& a, const double* f, double* ddq, double* dvl,
                                 double* dwl, double* T);
hipError_t launch_k_warm(hipStream_t st, const KArgs& a);
hipError_t launch_k_env(hipStream_t st, const KArgs& a, double* lhs, double* rhs, int* nrow, unsigned char* col,
                        double* md);
// wide: 16-byte units (ck_wide); one wavefront per record
hipError_t launch_k_ckpt_gather(bool wide, hipStream_t st, const CkArgs& c, const int* list, int count, double* out);
hipError_t launch_k_ckpt_scatter(bool wide, hipStream_t st, const CkArgs& c, const double* in, const int* recs,
                                 const int* scen, int base, int count);

}  // namespace dat
