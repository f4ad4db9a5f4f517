// dat_handle.hpp -- what the host units of libdat.so share: the handle and its member structs, the per-scenario
// array lists, the error path, and the helpers that more than one unit calls (allocation, side streams, the handle as
// kernel arguments, scratch buffers, counter reads, the checkpoint record's arguments).  Host code: dat.hip and the
// dat_h_*.hip beside it include it, no kernel unit does.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/dat.h"
#include "dat_ckpt.hpp"
#include "dat_kargs.hpp"
#include "dat_launch.hpp"
#include "dat_modes.hpp"

using namespace dat;

// the calling thread's message for dat_last_error (dat.hip holds it); returns -1
int fail(const std::string& m);

#define HIPCHK(x)                                                                 \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

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
  int force_rms = -1;            // dat_debug_row_modes: k_cadmm's row modes (rm_pack) instead of the rule's; -1: the rule's
  int tail_prev = TAIL_PREV, tail_pass = TAIL_PASS;  // the tail rule with a forest (dat_debug_tail_rule: another pair)
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

// the features the handle holds open, as the set the exclusion table speaks of (dat_modes.hpp: refusal)
inline unsigned open_features(const dat_handle* h) {
  return (h->log.open ? feat_bit(FEAT_LOG) : 0u) | (h->ep.open ? feat_bit(FEAT_EPISODES) : 0u) |
         (h->track ? feat_bit(FEAT_TRACKING) : 0u) | (h->plant == DAT_PLANT_RP ? feat_bit(FEAT_PLANT_RP) : 0u);
}
// 0 where `caller` may open the feature / do the action `want` on the handle, else the table's refusal as the error
// (among: the open features the caller asks about)
inline int admit(const dat_handle* h, const char* caller, int want, unsigned among = ~0u) {
  const std::string no = refusal(caller, want, open_features(h) & among);
  return no.empty() ? 0 : fail(no);
}

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

// C-ADMM scenario slots per k_cadmm wavefront (dat.hip)
int cadmm_slots(const dat_handle* h, int B, int n);

template <typename T>
int dalloc(dat_handle* h, T** p, size_t count) {
  *p = nullptr;
  if (count == 0) return 0;
  HIPCHK(hipMalloc((void**)p, count * sizeof(T)));
  HIPCHK(hipMemsetAsync(*p, 0, count * sizeof(T), h->stream));
  h->allocs.push_back(*p);
  return 0;
}

inline void dfree(dat_handle* h, void* p) {
  if (!p) return;
  for (auto& q : h->allocs)
    if (q == p) q = nullptr;
  (void)hipFree(p);
}

// err, the residual record (record_err handles only; dat_set_max_iter regrows it): elements per scenario
inline size_t err_extent(int max_iter) { return (size_t)max_iter + 1; }
// elements per scenario of the array behind the handle's member *member, as the lists state it
inline size_t extent_of(const dat_handle* h, const void* member) {
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
inline SubRange sub_range(int batch, int s, int S) {
  const long long B = batch;
  const int off = (int)(B * s / S);
  return {off, (int)(B * (s + 1) / S) - off};
}

// a timed event of the handle's, made on first use
inline hipError_t own_event(dat_handle* h, hipEvent_t* e) {
  if (*e) return hipSuccess;
  const hipError_t r = hipEventCreate(e);
  if (r == hipSuccess) h->events.push_back(*e);
  return r;
}

// The side stream *s with nev events: got, or made on first use.  A failure leaves *s empty and no sticky error:
// the caller falls back (no tail routing, the serial schedule) or reports it.
inline hipError_t side_get(dat_handle* h, side_stream* s, int nev) {
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
inline void side_release(dat_handle* h, side_stream* s) {
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

// the handle as kernel arguments: a projection, nothing is created.  route: the call's plan routes the tail
// (LoopPlan::tail_route; without it the wedged scenarios go through k_cadmm's hand-over, same results)
inline KArgs kargs(const dat_handle* h, bool route = false) {
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
  a.tail_prev = h->nforest > 0 ? h->tail_prev : INT_MAX;
  a.tail_pass = h->nforest > 0 ? h->tail_pass : INT_MAX;
  a.route = route;
  a.tmode = 0;
#ifdef DAT_NO_TAIL  // A/B builds only (tools/build_var.sh): the round-5 schedule, no tail rule
  a.tail_prev = a.tail_pass = INT_MAX;
  a.route = 0;
#endif
  return a;
}

// kernel arguments of sub-batch s, the scenarios r (dat_set_sub_batches; the whole batch: those of kargs): every
// per-scenario array offset by the lists' extents (the env-row image then a disjoint block of the SoA buffer,
// stride r.count n), the class table its own; counters shared (atomics)
template <class T>
T* offp(T* p, size_t k) { return p ? p + k : p; }
inline KArgs sub_kargs(const dat_handle* h, SubRange r, int s, bool route = false) {
  KArgs a = kargs(h, route);
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
inline int read_words(dat_handle* h, const unsigned long long* src, unsigned long long* out, int count) {
  HIPCHK(hipSetDevice(h->cfg.device));
  std::fill(out, out + count, 0ull);
  if (!src) return 0;
  HIPCHK(hipMemcpyAsync(out, src, sizeof(*out) * count, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
// ... each word to its destination, where that is not null
inline int read_words(dat_handle* h, const unsigned long long* src, std::initializer_list<long long*> out) {
  unsigned long long c[8];
  if (read_words(h, src, c, (int)out.size())) return -1;
  int k = 0;
  for (long long* p : out) {
    if (p) *p = (long long)c[k];
    ++k;
  }
  return 0;
}

// ---- the checkpoint record, for the checkpoints and the episodes' respawn -------------------------------------------
// the handle's record as the copy kernels' arguments: the table of dat_ckpt.hpp with the handle's arrays put in
inline dat::CkArgs ck_args(const dat_handle* h) {
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
inline bool ck_wide(const dat::CkArgs& c) {
  bool even = c.ints_off % 2 == 0 && c.words % 2 == 0;
  for (int k = 0; k < c.nf; ++k) even = even && c.w[k] % 2 == 0 && c.off[k] % 2 == 0;
  return even;
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

// ---- what dat.hip calls of the units beside it ----------------------------------------------------------------------
// dat_h_log.hip: the open log's kernel arguments for the sub-batch of scenarios [off, ...) at the current clock;
// whether a dat_closed_loop call of hl_steps fits the log's capacity; the log's buffers freed and the log closed
LogArgs log_args(const dat_handle* h, int off = 0);
int log_admit(const dat_handle* h, int hl_steps);
void log_free(dat_handle* h);
// dat_h_episode.hip: the open episodes' kernel arguments for the sub-batch of scenarios [off, ...) at the step of
// tick `tick`
EpArgs ep_args(const dat_handle* h, int off, long long tick);
