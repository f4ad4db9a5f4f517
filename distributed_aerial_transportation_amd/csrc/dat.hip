// dat.hip -- the host side of libdat.so: the handle, the per-scenario array lists, the side streams, the step chain
// and the closed loop's schedules, the log, the checkpoints, the episodes, and every dat_* export of the C-ABI
// (include/dat.h).
// No kernel lives here: the gfx950 kernels are the units beside it (dat_launch.hpp lists them, dat_cent.hip the
// centralized one), reached through their launchers, and this file says in what order, on which stream and between
// which events they run.
//
// Kernels (all fp64, no MFMA -- every contraction is <= 6 wide):
//   k_cadmm    C-ADMM control step: one 64-lane wavefront holds floor(64/n) scenarios x n agents,
//              one lane per agent QP; the whole ADMM loop (reference control/rqp_cadmm.py:631-675)
//              runs on chip: agent QPs (ipm_solve), consensus mean / residual through LDS, dual
//              update; per-scenario convergence masks (dat_cadmm_drain.hpp).
//   k_dd_setup DD quasi-Newton matrix H = A Q^-1 A' and its inverse per scenario, in LDS
//              (control/rqp_dd.py:513-555, 634-657): dat_k_dd.hip.
//   k_dd       DD control step: prices, agent QPs, consensus error, dual ascent through H^-1
//              (control/rqp_dd.py:659-752): dat_dd_drain.hpp.
//   k_cent     centralized QP, one lane group per scenario and one lane per agent's force
//              (control/rqp_centralized.py:436-448): dat_cent.hip.
//   k_rollout_agents  low-level SO(3) law + dynamics + Lie integration, one lane per agent (dat_k_step.hip, as the
//              next two).
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
#include <string>
#include <vector>
#include <algorithm>
#include <chrono>

#include "../../include/dat.h"
#include "dat_cadmm_lds.hpp"
#include "dat_ckpt.hpp"
#include "dat_episode_host.hpp"
#include "dat_kargs.hpp"
#include "dat_launch.hpp"

using namespace dat;

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

// lg: the open log's arguments at this launch (dat_closed_loop), or null: the plain kernel
// adv: the pass of the closed loop's advance overlap (ADV_ALL: every scenario)
// ep: the open episodes' arguments at this launch (dat_closed_loop), or null
hipError_t launch_rollout(const KArgs& a, int B, hipStream_t stream, int steps, double dt, const double* fdes,
                          const LogArgs* lg = nullptr, int adv = ADV_ALL, const EpArgs* ep = nullptr) {
  const int G = 64 / a.n;
  return launch_k_rollout_agents(lg, adv, (B + G - 1) / G, stream, a, steps, dt, fdes, ep);
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
// The open episodes (dat_episode_begin .. dat_episode_end): the rules, the pool's records and the outcome table in
// HBM, and the counters the kernels append through (EpCounter).  The accumulators are an array of the handle's
// table (epacc), allocated with the others.
struct dat_episodes {
  bool open = false;
  dat_episode_rules rules = {};
  double* pool = nullptr;
  int P = 0;
  double* table = nullptr;
  int cap = 0;
  unsigned long long* cnt = nullptr;
};
struct dat_handle {
  dat_log log;
  dat_episodes ep;
  EpAcc* epacc = nullptr;
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
  // The tracking law (dat_set_tracking; null: the forest law), the clock (simulation steps since dat_create;
  // dat_set_clock) and the plant dat_closed_loop rolls out (dat_set_plant).  Settings, like parameters: no
  // checkpoint carries them.
  double* track = nullptr;
  int track_pp = 0;
  long long clock = 0;
  int plant = DAT_PLANT_RQP;
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
#define DAT_ARRAYS_ALL(X, n) X(counter, 1) X(iters, 1) X(acc, 6) X(qstatus, n) X(mind, 1) X(col, 1) X(epacc, 1)
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
  a.track = h->track;
  a.track_pp = h->track_pp;
  a.tick = h->clock;
  a.dt = c.dt;
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
  const auto kc = adv ? launch_k_cadmm_adv : launch_k_cadmm;  // (forest, blocks, LDS bytes, stream, arguments)
  const auto kt = launch_k_cadmm_tail;
  if (h->nforest > 0) {
    if (a.route) {
      KArgs t = r;
      t.tmode = 1;
      const hipStream_t ts = h->tail.st;
      HIPCHK(hipEventRecord(h->tail.ev[0], st));
      HIPCHK(hipStreamWaitEvent(ts, h->tail.ev[0], 0));
      HIPCHK(kt(true, TAIL_BLOCKS, cadmm_tail_lds_bytes(a.n, NCLS - 1), ts, t));
      HIPCHK(hipEventRecord(h->tail.ev[1], ts));
    }
    HIPCHK(kc(true, blocks, cadmm_lds_bytes(a.n, a.G, NCLS - 1), st, a));
    HIPCHK(kt(true, TAIL_BLOCKS, cadmm_tail_lds_bytes(r.n, NCLS - 1), st, r));
    if (a.route) HIPCHK(hipStreamWaitEvent(st, h->tail.ev[1], 0));
  } else {
    HIPCHK(kc(false, blocks, cadmm_lds_bytes(a.n, a.G, 0), st, a));
    HIPCHK(kt(false, TAIL_BLOCKS, cadmm_tail_lds_bytes(r.n, 0), st, r));
  }
  return 0;
}

// The DD kernels of a step: the quasi-Newton matrix (k_dd_setup, the instantiation and its LDS limit by n:
// dat_k_dd.hip), the sort by the previous step's iterations, the drain
int launch_dd(const dat_handle* h, const KArgs& a, hipStream_t st, hipEvent_t ek) {
  const int n = a.n, B = a.B;
  HIPCHK(launch_k_dd_setup(B, dd_setup_lds(n), st, a));
  HIPCHK(launch_k_dd_key(st, a));
  HIPCHK(launch_k_bucket(st, B, (const int*)a.need, a.slist, a.scount));
  HIPCHK(hipEventRecord(ek, st));
  const bool env = h->nforest > 0;
  const int G = 64 / n, blocks = std::min((B + G - 1) / G, h->persistent_blocks);
  HIPCHK((env ? launch_k_dd_env : launch_k_dd)(blocks, dd_lds(n, env), st, a));
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
  if (a.track_pp) a.track = offp(a.track, o * DAT_TRACK_SIZE);
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

// the open episodes' kernel arguments for the sub-batch of scenarios [off, ...) at the step of tick `tick`
dat::CkArgs ck_args(const dat_handle* h);  // (below, with the checkpoints)
EpArgs ep_args(const dat_handle* h, int off, long long tick) {
  const dat_episodes& e = h->ep;
  EpArgs a;
  a.rules = e.rules;
  a.pool = e.pool;
  a.P = e.P;
  a.batch = h->cfg.batch;
  a.off = off;
  a.hl_every = h->cfg.hl_every;
  a.tick = tick;
  a.table = e.table;
  a.cap = e.cap;
  a.cnt = e.cnt;
  a.ck = ck_args(h);
  return a;
}

void ep_free(dat_handle* h) {
  dat_episodes& e = h->ep;
  dfree(h, e.pool);
  dfree(h, e.table);
  dfree(h, e.cnt);
  e = dat_episodes();
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
hipError_t launch_inputs(const dat_handle* h, const Sub& u, int mode = ADV_ALL, int parts = IN_DESIRED | IN_ENV) {
  const int B = u.a.B, G = 64 / u.a.n;
  hipError_t e = hipSuccess;
  if (parts & IN_DESIRED) e = launch_k_desired(mode, u.st, u.a, (double*)u.a.acc);
  if (e == hipSuccess && (parts & IN_ENV) && h->cfg.mode == DAT_MODE_CADMM)
    e = launch_k_env_class(mode, (B + G - 1) / G, u.st, u.a);
  return e;
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
      HIPCHK(launch_k_bucket(u.st, a.B, (const int*)a.need, a.slist, a.scount));
    else if (u.ktab) {
      HIPCHK(launch_k_bucket_scatter(mode, u.st, a.B, (const int*)a.need, a.slist, a.scount, (const int*)a.adv, stamp,
                                     u.ktab, u.kzero));
      ++h->n_scatter;
    } else
      HIPCHK(launch_k_bucket_adv(mode, u.st, a.B, (const int*)a.need, a.slist, a.scount, (const int*)a.adv, stamp));
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
  HIPCHK(launch_inputs(h, u, ADV_ALL, IN_ENV));
  return launch_control(h, u);
}

// The rollout of a closed-loop step in the pass `mode`; with a log open the recording kernel, at the log's clock
// (sub-batch streams run unsynchronised: the record index is the sub-batch's own step count).
// With episodes open the kernel with the episode flag, at the step's tick (u.a.tick).
hipError_t launch_step_rollout(const dat_handle* h, const Sub& u, int mode = ADV_ALL) {
  const LogArgs lg = h->log.open ? log_args(h, u.off) : LogArgs();
  const EpArgs ep = h->ep.open ? ep_args(h, u.off, u.a.tick) : EpArgs();
  return launch_rollout(u.a, u.a.B, u.st, h->cfg.hl_every, h->cfg.dt, (const double*)u.a.fdes,
                        h->log.open ? &lg : nullptr, mode, h->ep.open ? &ep : nullptr);
}

// A pass (ADV_EARLY / ADV_REST) of the overlap and the pipeline: the rollout of the step and, with `inputs`, the next
// step's inputs of the scenarios it advanced.  One launch of k_advance where the switch is on (these schedules run
// C-ADMM on one sub-batch with no log open: advance_ready), else the three kernels of the step chain.
// fused_ready is the one statement of where k_advance runs: the passes go by it here, and the pipeline hands out key
// tables (Sub::kc_lo / ktab) by it, so a sort reads a key table only behind passes that counted into it.  A pass
// that is given a table and would not count (the three kernels do not) is an error, not a silently empty list.
bool fused_ready(const dat_handle* h) { return h->fused_on && h->cfg.mode == DAT_MODE_CADMM && !h->log.open; }
// u.a.tick is the tick of the step the pass rolls out; the inputs it computes are the next step's and carry that
// step's tick, one HL period on.
int launch_advance(const dat_handle* h, const Sub& u, int mode, bool inputs) {
  Sub nx = u;
  nx.a.tick = u.a.tick + h->cfg.hl_every;
  if (inputs && mode != ADV_ALL && fused_ready(h)) {
    const int G = 64 / u.a.n;
    const EpArgs ep = h->ep.open ? ep_args(h, u.off, u.a.tick) : EpArgs();
    HIPCHK(launch_k_advance(mode, (u.a.B + G - 1) / G, u.st, nx.a, h->cfg.hl_every, h->cfg.dt, (const double*)u.a.fdes,
                            (double*)u.a.acc, u.kc_lo, u.kc_hi, h->ep.open ? &ep : nullptr));
    ++h->n_advance;
    return 0;
  }
  if (inputs && u.kc_lo) return fail("launch_advance: a key table was handed to a pass that runs the three kernels");
  HIPCHK(launch_step_rollout(h, u, mode));
  if (inputs) HIPCHK(launch_inputs(h, nx, mode));
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
  HIPCHK(launch_inputs(h, base));
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
    base.a.tick = h->clock + (long long)k * h->cfg.hl_every;  // step k's tick (launch_advance: its inputs are step k + 1's)
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
  h->clock += (long long)hl_steps * h->cfg.hl_every;
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
dat::CkArgs ck_args(const dat_handle* h) {
  dat::CkArgs c;
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
bool ck_wide(const dat::CkArgs& c) {
  bool even = c.ints_off % 2 == 0 && c.words % 2 == 0;
  for (int k = 0; k < c.nf; ++k) even = even && c.w[k] % 2 == 0 && c.off[k] % 2 == 0;
  return even;
}

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
  // the tail's workgroup may exceed the default 64 KB of dynamic LDS (the limit: dat_k_cadmm_tail.hip)
  if (c.mode == DAT_MODE_CADMM && tail_lds_limit_raise(c.device, c.n) != hipSuccess) {
    dat_destroy(h);
    return fail("dat_create: tail kernel LDS attribute");
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
  h->ep = dat_episodes();  // (its buffers went with the list)
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
  HIPCHK(launch_k_warm(h->stream, a));
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
  const dat::CkArgs c = ck_args(h);
  const size_t words = (size_t)count * c.words;
  if (ck_grow(h, &h->ck_stage, &h->ck_stage_cap, words)) return -1;
  if (scenarios) {
    if (ck_grow(h, &h->ck_list, &h->ck_list_cap, (size_t)count)) return -1;
    HIPCHK(hipMemcpyAsync(h->ck_list, scenarios, sizeof(int) * count, hipMemcpyHostToDevice, h->stream));
  }
  const int* list = scenarios ? h->ck_list : nullptr;
  HIPCHK(hipEventRecord(h->e0, h->stream));
  HIPCHK(launch_k_ckpt_gather(ck_wide(c), h->stream, c, list, count, h->ck_stage));
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
  if (h->ep.open)
    return fail("dat_checkpoint_load: episodes are open on the handle (a loaded scenario would not be the episode its "
                "slot is recorded to run): dat_episode_end first; nothing was written");
  std::string m;
  long long lo = 0, hi = 0;
  if (ck_check_load(h->cfg.mode, h->cfg.n, h->cfg.batch, blob, bytes, records, scenarios, count, &lo, &hi, &m))
    return fail(m);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t s : h->streams) HIPCHK(hipStreamSynchronize(s));
  const dat::CkArgs c = ck_args(h);
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
  HIPCHK(launch_k_ckpt_scatter(ck_wide(c), st, c, (const double*)h->ck_stage, (const int*)recs, (const int*)scen,
                               (int)lo, count));
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
    HIPCHK(launch_inputs(h, u, ADV_ALL, IN_DESIRED));
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
  HIPCHK(launch_rollout(a, (int)B, h->stream, steps, h->cfg.dt, (const double*)h->fdes));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->clock += steps;
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
// Every launch that computes a desired acceleration carries the tick it is evaluated at (KArgs::tick; the tracking law,
// dat_set_tracking): step k's is clock + k hl_every, and the passes that compute step k + 1's inputs carry that
// step's (launch_advance).  The call advances the clock by hl_steps x hl_every.
// With episodes open (dat_episode_begin) every pass that rolls scenarios out launches the kernel with the episode flag
// (launch_step_rollout, launch_advance): a scenario's episode step stands between the pass's gate and its rollout, the
// early pass leaves an ending scenario to the rest pass, and the schedules stay what they are.
// With the rigid-payload plant (dat_set_plant, centralized handles) a step is k_cent and k_rp_advance, which runs the
// payload's hl_every steps and the next step's desired acceleration, on the serial schedule.
// What the early pass may touch while the drain runs: a finished scenario's state, acc, env rows / mask, sort key
// and rotation counter are read by the drain only when a slot takes the scenario (the refill; ksteps == 1 here),
// so they may be overwritten; its f_des, iters and ipmx were stored write-through before the stamp and are read
// past the caches; everything else the early kernels read dates from before the drain's launch.
// With sub-batches hl_ms is the whole call's device time (the sub-batches' kernels overlap) and cadmm_ms the sum of
// the k_cadmm launch spans (S launches per HL step: dat_get_kernel_ms / (hl_steps S) is one launch).
int dat_closed_loop(dat_handle* h, int hl_steps) {
  if (!h) return fail("null handle");
  const bool rp = h->plant == DAT_PLANT_RP;
  if (rp && h->log.open)
    return fail("dat_closed_loop: the log does not record the rigid-payload plant (DAT_PLANT_RP) yet: close the log");
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
      v.a.tick = h->clock + (long long)k * h->cfg.hl_every;
      if (rp) {  // k_cent, then the payload's steps and the next step's desired acceleration in one launch
        if (k == 0) HIPCHK(launch_inputs(h, v, ADV_ALL, IN_DESIRED));
        if (launch_step(h, v, S == 1)) return -1;
        KArgs nx = v.a;
        nx.tick = v.a.tick + h->cfg.hl_every;
        HIPCHK(launch_k_rp_advance(v.st, nx, h->cfg.hl_every, h->cfg.dt, (const double*)v.a.fdes,
                                   k + 1 < hl_steps ? (double*)v.a.acc : nullptr));
      } else if (!overlap) {
        HIPCHK(launch_inputs(h, v, ADV_ALL, IN_DESIRED));
        if (launch_step(h, v, S == 1)) return -1;
        HIPCHK(launch_step_rollout(h, v));
      } else {
        if (step_begin(h, v)) return -1;
        if (k == 0) HIPCHK(launch_inputs(h, v));
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
  if (hl_steps > 0) h->clock += (long long)hl_steps * h->cfg.hl_every;
  return 0;
}

// ---- the tracking law, the clock and the plant ------------------------------------------------------------------
int dat_set_tracking(dat_handle* h, const double* rec, int per_scenario) {
  if (!h) return fail("dat_set_tracking: null handle");
  if (rec && h->ep.open)
    return fail("dat_set_tracking: episodes do not run under tracking records yet: dat_episode_end first; the law in "
                "force is unchanged");
  const size_t count = per_scenario ? (size_t)h->cfg.batch : 1;
  if (rec) {  // checked on the host before anything is copied or launched
    static const char* const names[DAT_TRACK_SIZE] = {"CX", "CY", "RADIUS", "HEIGHT", "FREQ", "T0", "KP", "KV",
                                                      "AMAX", "WAMP", "WZ", "reserved"};
    for (size_t k = 0; k < count; ++k) {
      const int bad = track_record_bad_field(rec + k * DAT_TRACK_SIZE);
      if (bad >= 0)
        return fail("dat_set_tracking: record " + std::to_string(k) + ": field " + names[bad] + " = " +
                    std::to_string(rec[k * DAT_TRACK_SIZE + bad]) +
                    " (every field must be finite; RADIUS, FREQ, KP, KV >= 0); the law in force is unchanged");
    }
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t s : h->streams) HIPCHK(hipStreamSynchronize(s));
  double* fresh = nullptr;
  if (rec) {
    if (dalloc(h, &fresh, count * DAT_TRACK_SIZE)) return -1;
    HIPCHK(hipMemcpyAsync(fresh, rec, sizeof(double) * count * DAT_TRACK_SIZE, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  dfree(h, h->track);
  h->track = fresh;
  h->track_pp = rec && per_scenario ? 1 : 0;
  return 0;
}

int dat_set_clock(dat_handle* h, long long clock) {
  if (!h) return fail("dat_set_clock: null handle");
  if (clock < 0) return fail("dat_set_clock: negative clock " + std::to_string(clock) + " (simulation steps, >= 0)");
  h->clock = clock;
  return 0;
}

int dat_get_clock(dat_handle* h, long long* clock) {
  if (!h || !clock) return fail("dat_get_clock: null argument");
  *clock = h->clock;
  return 0;
}

int dat_set_plant(dat_handle* h, int plant) {
  if (!h) return fail("dat_set_plant: null handle");
  if (plant != DAT_PLANT_RQP && plant != DAT_PLANT_RP) return fail("dat_set_plant: bad plant " + std::to_string(plant));
  if (plant == DAT_PLANT_RP && h->cfg.mode != DAT_MODE_CENTRALIZED)
    return fail("dat_set_plant: the rigid-payload plant (DAT_PLANT_RP) runs on centralized handles only");
  if (plant == DAT_PLANT_RP && h->log.open)
    return fail("dat_set_plant: the log does not record the rigid-payload plant (DAT_PLANT_RP) yet: close the log");
  if (plant == DAT_PLANT_RP && h->ep.open)
    return fail("dat_set_plant: episodes do not run on the rigid-payload plant (DAT_PLANT_RP) yet: dat_episode_end first");
  h->plant = plant;
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
  HIPCHK(launch_k_env(h->stream, a, dl, dr, dn, dc, dm));
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
  dat::AgentQPArgs q;
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
  HIPCHK(launch_k_agent_qp(h->stream, a, q));
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
  HIPCHK(launch_k_low_level(h->stream, a, (const double*)h->fdes, df, dm));
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
  HIPCHK(launch_k_rp_rollout(h->stream, a, steps, h->cfg.dt, (const double*)h->fdes));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->clock += steps;
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
  HIPCHK(launch_k_pmrl_rollout((B + G - 1) / G, h->stream, a, steps, nf, h->cfg.dt, (const double*)h->pmrl_buf));
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
  HIPCHK(launch_k_pmrl_forward((B + G - 1) / G, h->stream, a, (const double*)(d + of), d + oq, d + ov, d + ow, d + oT));
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
  if (h->ep.open) return fail("dat_log_begin: the log does not record episodes yet: dat_episode_end first");
  if (h->plant == DAT_PLANT_RP)
    return fail("dat_log_begin: the log does not record the rigid-payload plant (DAT_PLANT_RP) yet");
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

// ---- episodes --------------------------------------------------------------------------------------------------
void dat_episode_default_rules(dat_episode_rules* r) {
  if (!r) return;
  memset(r, 0, sizeof(*r));
  r->goal_x = HUGE_VAL;
  r->bound = HUGE_VAL;
  r->wrap = 1;
}

int dat_episode_begin(dat_handle* h, const dat_episode_rules* rules, const void* pool_blob, long long bytes,
                      int capacity) {
  if (!h) return fail("dat_episode_begin: null handle");
  if (h->ep.open) return fail("dat_episode_begin: episodes are already open (dat_episode_end first)");
  if (h->log.open) return fail("dat_episode_begin: the log does not record episodes yet: dat_log_end first");
  if (h->plant == DAT_PLANT_RP)
    return fail("dat_episode_begin: episodes do not run on the rigid-payload plant (DAT_PLANT_RP) yet");
  if (h->track) return fail("dat_episode_begin: episodes do not run under tracking records yet: dat_set_tracking(NULL) first");
  std::string m;
  int P = 0;
  if (ep_check_begin(h->cfg.mode, h->cfg.n, rules, pool_blob, bytes, capacity, &P, &m)) return fail(m);
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t s : h->streams) HIPCHK(hipStreamSynchronize(s));
  const int B = h->cfg.batch;
  const dat::CkArgs c = ck_args(h);
  const size_t words = (size_t)P * c.words;
  // slot s runs record s mod P first (its episode 0); without wrap a slot beyond the pool is idle from the start
  std::vector<EpAcc> acc((size_t)B);
  std::vector<int> recs((size_t)B);
  unsigned long long cnt[EPC_WORDS] = {0};
  for (int s = 0; s < B; ++s) {
    int idle = 0;
    recs[(size_t)s] = episode_record(s, 0, B, P, rules->wrap, &idle);
    episode_start(acc[(size_t)s], recs[(size_t)s], h->clock, 0, idle);
    cnt[EPC_IDLE] += idle ? 1 : 0;
  }
  dat_episodes& e = h->ep;
  if (dalloc(h, &e.pool, words) || dalloc(h, &e.table, (size_t)std::max(capacity, 1) * DAT_EP_WORDS) ||
      dalloc(h, &e.cnt, (size_t)EPC_WORDS) || ck_grow(h, &h->ck_list, &h->ck_list_cap, (size_t)B)) {
    (void)hipGetLastError();
    ep_free(h);
    return -1;
  }
  const hipStream_t st = h->stream;
  hipError_t r = hipMemcpyAsync(e.pool, (const char*)pool_blob + DAT_CK_HEADER_BYTES, sizeof(double) * words,
                                hipMemcpyHostToDevice, st);
  if (r == hipSuccess) r = hipMemcpyAsync(e.cnt, cnt, sizeof(cnt), hipMemcpyHostToDevice, st);
  if (r == hipSuccess) r = hipMemcpyAsync(h->epacc, acc.data(), sizeof(EpAcc) * (size_t)B, hipMemcpyHostToDevice, st);
  if (r == hipSuccess) r = hipMemcpyAsync(h->ck_list, recs.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice, st);
  if (r == hipSuccess)
    r = launch_k_ckpt_scatter(ck_wide(c), st, c, (const double*)e.pool, (const int*)h->ck_list, nullptr, 0, B);
  if (r == hipSuccess) r = hipStreamSynchronize(st);
  if (r != hipSuccess) {
    ep_free(h);
    return fail(std::string("dat_episode_begin: ") + hipGetErrorString(r));
  }
  e.rules = *rules;
  e.P = P;
  e.cap = capacity;
  e.open = true;
  return 0;
}

int dat_episode_counts(dat_handle* h, long long* ended, long long* held, long long* lost, long long* idle) {
  if (!h) return fail("dat_episode_counts: null handle");
  if (!h->ep.open) return fail("dat_episode_counts: no episodes open");
  unsigned long long c[EPC_WORDS];
  if (read_words(h, h->ep.cnt, c, EPC_WORDS)) return -1;
  if (ended)
    for (int k = 0; k < DAT_EP_NREASON; ++k) ended[k] = (long long)c[EPC_ENDED + k];
  if (held) *held = (long long)std::min<unsigned long long>(c[EPC_COUNT], (unsigned long long)h->ep.cap);
  if (lost) *lost = (long long)c[EPC_LOST];
  if (idle) *idle = (long long)c[EPC_IDLE];
  return 0;
}

int dat_episode_read(dat_handle* h, int first, int count, int* slot, int* episode, int* record, int* reason,
                     long long* start_tick, long long* end_tick, int* steps, int* iter_sum, int* iter_max,
                     int* full_steps, int* stall_run, double* min_env_dist, double* xl, double* vl) {
  if (!h) return fail("dat_episode_read: null handle");
  if (!h->ep.open) return fail("dat_episode_read: no episodes open");
  long long held = 0;
  if (dat_episode_counts(h, nullptr, &held, nullptr, nullptr)) return -1;
  std::string m;
  if (ep_check_read(first, count, held, &m)) return fail(m);
  if (count == 0) return 0;
  std::vector<double> w((size_t)count * DAT_EP_WORDS);
  HIPCHK(hipMemcpyAsync(w.data(), h->ep.table + (size_t)first * DAT_EP_WORDS, sizeof(double) * w.size(),
                        hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < (size_t)count; ++k) {
    const double* r = w.data() + k * DAT_EP_WORDS;
    const auto ints = [&](int word, int* lo, int* hi) {
      int v[2];
      memcpy(v, r + word, sizeof(v));
      if (lo) lo[k] = v[0];
      if (hi) hi[k] = v[1];
    };
    ints(DAT_EP_SLOT, slot, episode);
    ints(DAT_EP_RECORD, record, reason);
    ints(DAT_EP_STEPS, steps, iter_sum);
    ints(DAT_EP_ITMAX, iter_max, full_steps);
    ints(DAT_EP_RUN, stall_run, nullptr);
    if (start_tick) memcpy(start_tick + k, r + DAT_EP_START, 8);
    if (end_tick) memcpy(end_tick + k, r + DAT_EP_END, 8);
    if (min_env_dist) min_env_dist[k] = r[DAT_EP_MIND];
    if (xl) memcpy(xl + 3 * k, r + DAT_EP_XL, sizeof(double) * 3);
    if (vl) memcpy(vl + 3 * k, r + DAT_EP_VL, sizeof(double) * 3);
  }
  return 0;
}

int dat_episode_clear(dat_handle* h) {
  if (!h) return fail("dat_episode_clear: null handle");
  if (!h->ep.open) return fail("dat_episode_clear: no episodes open");
  static_assert(EPC_COUNT == 0 && EPC_LOST == 1, "the cursor and the lost count are cleared together");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemsetAsync(h->ep.cnt, 0, 2 * sizeof(unsigned long long), h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int dat_episode_end(dat_handle* h) {
  if (!h) return fail("dat_episode_end: null handle");
  if (!h->ep.open) return fail("dat_episode_end: no episodes open");
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t s : h->streams) HIPCHK(hipStreamSynchronize(s));
  ep_free(h);
  return 0;
}

int dat_episode_slots(dat_handle* h, int* record, int* episodes, int* steps, int* idle) {
  if (!h) return fail("dat_episode_slots: null handle");
  if (!h->ep.open) return fail("dat_episode_slots: no episodes open");
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<EpAcc> acc((size_t)h->cfg.batch);
  HIPCHK(hipMemcpyAsync(acc.data(), h->epacc, sizeof(EpAcc) * acc.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t s = 0; s < acc.size(); ++s) {
    if (record) record[s] = acc[s].record;
    if (episodes) episodes[s] = acc[s].episodes;
    if (steps) steps[s] = acc[s].steps;
    if (idle) idle[s] = acc[s].idle;
  }
  return 0;
}

int dat_get_episode_respawns(dat_handle* h, long long* early, long long* rest, long long* deferred) {
  if (!h) return fail("dat_get_episode_respawns: null handle");
  if (!h->ep.open) return fail("dat_get_episode_respawns: no episodes open");
  static_assert(EPC_DEFERRED == EPC_RESPAWN + 2, "the three words are read together");
  return read_words(h, h->ep.cnt + EPC_RESPAWN, {early, rest, deferred});
}

}  // extern "C"
