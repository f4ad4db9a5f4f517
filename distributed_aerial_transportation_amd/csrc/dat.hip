// dat.hip -- the host side of libdat.so: the handle's lifecycle, its setters and getters, the step chain, the closed
// loop's schedules and the one-shot entry points of the C-ABI (include/dat.h).  The handle itself and what the host
// units share are dat_handle.hpp's; the log, the episodes and the checkpoints are the units dat_h_log.hip,
// dat_h_episode.hip and dat_h_ckpt.hip; which features exclude which and which schedule a call runs are
// dat_modes.hpp's.
// No kernel lives here: the gfx950 kernels are the units beside it (dat_launch.hpp lists them, dat_cent.hip the
// centralized one), reached through their launchers, and this file says in what order, on which stream and between
// which events they run.
#include <cmath>
#include <chrono>

#include "dat_handle.hpp"
#include "dat_cadmm_host.hpp"
#include "dat_cadmm_lds.hpp"

namespace {
thread_local std::string g_err;
}  // namespace

int fail(const std::string& m) {
  g_err = m;
  return -1;
}

namespace {

// lg: the open log's arguments at this launch (dat_closed_loop), or null: the plain kernel
// adv: the pass of the closed loop's advance overlap (ADV_ALL: every scenario)
// ep: the open episodes' arguments at this launch (dat_closed_loop), or null
hipError_t launch_rollout(const KArgs& a, int B, hipStream_t stream, int steps, double dt, const double* fdes,
                          const LogArgs* lg = nullptr, int adv = ADV_ALL, const EpArgs* ep = nullptr) {
  const int G = 64 / a.n;
  return launch_k_rollout_agents(lg, adv, (B + G - 1) / G, stream, a, steps, dt, fdes, ep);
}

}  // namespace

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

// the C-ADMM drain of one control step: k_cadmm (env classes 3, 2, 1, 0) with a forest, k_cadmm0 without.
// k_cadmm_tail: one scenario slot per block (G = 1).  Its scenarios are few -- stalled ADMM loops next to trees,
// 101 sequential passes -- and a slot of its own per scenario keeps one scenario's pass from waiting for the
// slowest agent QP of the others'.  With a forest two launches: the tail-routed scenarios on the sub-batch's
// tail stream, started with k_cadmm (their lists are known after k_bucket), and the hand-over lists after
// k_cadmm on the step's stream, which then waits for the first.
constexpr int TAIL_BLOCKS = 256;
constexpr size_t CADMM_LDS_MAX = 64 * 1024;  // dynamic LDS of a k_cadmm workgroup without a raised limit
// (KArgs::done set: the ADV instantiations, dat_closed_loop's overlap)
int launch_cadmm(const dat_handle* h, const KArgs& a, int blocks, hipStream_t st) {
  KArgs r = a;
  r.G = 1;
  const bool adv = a.done != nullptr;
  const auto kc = adv ? launch_k_cadmm_adv : launch_k_cadmm;  // (forest, row modes, blocks, LDS bytes, stream, arguments)
  const auto kt = launch_k_cadmm_tail;
  // the row modes of the launch, stated once: the kernel instantiation and the carve's bytes both go by this word
  // (the rule's, cadmm_row_modes; dat_debug_row_modes: a forced one)
  const int rms = h->force_rms >= 0 ? h->force_rms : cadmm_row_modes(a.n, a.G);
  const int max_cls = h->nforest > 0 ? NCLS - 1 : 0;
  const size_t lds = cadmm_lds_bytes_of(a.n, a.G, max_cls, rms);
  if (!cadmm_rms_built(rms)) return fail("k_cadmm: no instantiation of the launch's row modes");
  if (lds > CADMM_LDS_MAX) return fail("k_cadmm: the forced row modes' carve exceeds a workgroup's dynamic LDS");
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
    HIPCHK(kc(true, rms, blocks, lds, st, a));
    HIPCHK(kt(true, TAIL_BLOCKS, cadmm_tail_lds_bytes(r.n, NCLS - 1), st, r));
    if (a.route) HIPCHK(hipStreamWaitEvent(st, h->tail.ev[1], 0));
  } else {
    HIPCHK(kc(false, rms, blocks, lds, st, a));
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
Sub sub_batch(const dat_handle* h, const LoopPlan& p, int s = 0, int S = 1) {
  const SubRange r = sub_range(h->cfg.batch, s, S);
  Sub u;
  u.st = h->sub[s].st;
  u.off = r.off;
  u.a = sub_kargs(h, r, s, p.tail_route);
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

// The handle's facts for the schedule rule (dat_modes.hpp: loop_plan), with the resources that are in place now.
// loop_steps: the HL steps of a dat_closed_loop call.  A call that runs no step sets out for the overlap at most, and
// a one-shot entry point (< 0) runs no schedule: it only routes the tail.
LoopFacts loop_facts(const dat_handle* h, int loop_steps) {
  LoopFacts f;
  f.mode = h->cfg.mode;
  f.nsub = h->nsub;
  f.forest = h->nforest > 0;
  f.log_open = h->log.open;
  f.record_err = h->cfg.record_err != 0;
  f.adv_on = h->adv_on && loop_steps >= 0;
  f.pipe_on = h->pipe_on && loop_steps > 0;
  f.fused_on = h->fused_on;
  f.fused_sort_build = DAT_FUSED_SORT != 0;
  f.have_words = h->qempty && h->qempty_dev && h->done && h->adv && h->advcnt;
  f.have_tail = h->tail.st != nullptr;
  f.have_advance = h->advance.st != nullptr;
  f.have_pipe = h->pipe.st != nullptr;
  f.have_lists = h->pipe_lists != nullptr;
  f.have_ktabs = h->ktabs != nullptr;
  return f;
}

// What every entry point that runs control steps starts with; *plan: what the call runs.  The rule says what the
// call would run if every resource were there; what that needs is made here on first use, in the order tail stream,
// advance stream, pipeline stream, its lists, its key tables (three streams beside the handle's: the four hardware
// queues).  A failure leaves no sticky error and ends the acquisitions, and the rule, asked again with what is there,
// steps down: pipeline -> overlap -> serial, no tail stream -> the hand-over inside k_cadmm, same results.
int step_entry(dat_handle* h, LoopPlan* plan, int loop_steps = -1) {
  if (!h->have_params) return fail("dat_set_params has not been called");
  HIPCHK(hipSetDevice(h->cfg.device));
  const LoopPlan want = loop_plan_wanted(loop_facts(h, loop_steps));
  if (want.tail_route) (void)side_get(h, &h->tail, 2);
  if (want.schedule >= SCHED_OVERLAP && side_get(h, &h->advance, 1) == hipSuccess && want.schedule == SCHED_PIPELINE) {
    const bool got = side_get(h, &h->pipe, 3) == hipSuccess &&
                     (h->pipe_lists || dalloc(h, &h->pipe_lists, (size_t)4 * h->cfg.batch) == 0) &&
                     (h->ktabs || dalloc(h, &h->ktabs, (size_t)4 * KT_INTS) == 0);
    if (!got) (void)hipGetLastError();
  }
  *plan = loop_plan(loop_facts(h, loop_steps));
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
// step's inputs of the scenarios it advanced.  One launch of k_advance where the call's plan says so (p.fused), else
// the three kernels of the step chain.  The pipeline hands out key tables (Sub::kc_lo / ktab) by the same plan
// (p.fused_sort), so a sort reads a key table only behind passes that counted into it.  A pass that is given a table
// and would not count (the three kernels do not) is an error, not a silently empty list.
// u.a.tick is the tick of the step the pass rolls out; the inputs it computes are the next step's and carry that
// step's tick, one HL period on.
int launch_advance(const dat_handle* h, const LoopPlan& p, const Sub& u, int mode, bool inputs) {
  Sub nx = u;
  nx.a.tick = u.a.tick + h->cfg.hl_every;
  if (inputs && mode != ADV_ALL && p.fused) {
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

// The overlapped schedules' host wait, after the drain of the step `serial` was enqueued: until the queue-empty word
// carries the serial (the drain's class-0 queue has been claimed empty), at the latest until the drain has ended
// (`end`; dat_debug_advance_split: always until then, so that every scenario's stamp is in place and the mask alone
// decides the split).  spin: called once per round of the wait (the pipeline's marks; the overlap passes nothing).
template <class F>
int wait_queue_empty(const dat_handle* h, int serial, hipEvent_t end, F spin) {
  const volatile int* const qe = h->qempty;
  for (;;) {
    bool hit = false;
    for (int k = 0; k < 256 && !hit; ++k) hit = !h->advmask && *qe == serial;
    spin();
    if (hit) break;
    const hipError_t q = hipEventQuery(end);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) HIPCHK(q);
  }
  (void)hipGetLastError();  // (a not-ready query is no error of the loop's)
  return 0;
}

// the next closed-loop step's stamp (0: the arrays' initial value, no step's stamp)
int next_serial(dat_handle* h) { return h->serial = h->serial == INT_MAX ? 1 : h->serial + 1; }

// sub_ev grown to n timed events: the drain event pairs of a call's steps (and sub-batches)
int sub_ev_reserve(dat_handle* h, size_t n) {
  while (h->sub_ev.size() < n) {
    hipEvent_t e = nullptr;
    HIPCHK(own_event(h, &e));
    h->sub_ev.push_back(e);
  }
  return 0;
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
int closed_loop_pipelined(dat_handle* h, const LoopPlan& p, int hl_steps) {
  const int B = h->cfg.batch;
  side_stream* const X[2] = {&h->advance, &h->pipe};
  if (sub_ev_reserve(h, 2 * (size_t)hl_steps)) return -1;
  Sub base = sub_batch(h, p);
  adv_args(h, base.a);
  // With the fused advance the passes count the keys of the sorts behind them (k_bucket_scatter).  The key tables of
  // the passes of step k: the main drain's `main(k)`, the rest drain's `rest(k)`, alternating with the step, each
  // zeroed by the sort of its kind one step earlier and all of them here, at the call's start (a call ends with the
  // last counting passes' tables sorted but not zeroed).
  const bool fsort = p.fused_sort;
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
    if (wait_queue_empty(h, serial, e1, [&] { mark(k); })) return -1;
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
    if (launch_advance(h, p, early, ADV_EARLY, more)) return -1;
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
    if (launch_advance(h, p, rest, ADV_REST, more)) return -1;
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
  // (the drain spans are the main drains': those of consecutive steps overlap)
  return account(h, h->e0, h->e1, h->sub_ev.data(), (size_t)hl_steps, hl_steps);
}

// The closed loop step by step: the serial schedule, the sub-batches and the overlap (dat_closed_loop)
int closed_loop_stepped(dat_handle* h, const LoopPlan& p, int hl_steps) {
  const bool rp = h->plant == DAT_PLANT_RP, overlap = p.schedule == SCHED_OVERLAP;
  const int S = h->nsub;
  const size_t ndrain = S > 1 && hl_steps > 0 ? (size_t)S * hl_steps : 0;
  Sub u[DAT_MAX_SUB];
  for (int s = 0; s < S; ++s) u[s] = sub_batch(h, p, s, S);
  if (overlap) adv_args(h, u[0].a);
  h->marks.assign(1, now_ms());
  if (S > 1) {  // a drain event pair per step and sub-batch; the sub-batch streams start after the handle's
    if (sub_ev_reserve(h, 2 * ndrain)) return -1;
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
        if (launch_control(h, v) || wait_queue_empty(h, h->serial, h->e1, [] {})) return -1;
        // the passes after the drain: the rollout, then (not after the call's last step) the next step's inputs
        Sub early = v;
        early.st = h->advance.st;
        if (launch_advance(h, p, early, ADV_EARLY, k + 1 < hl_steps)) return -1;
        HIPCHK(hipEventRecord(h->advance.ev[0], early.st));
        // (the rest pass is enqueued before the wait for the drain, so that its end finds it in the queue)
        HIPCHK(hipStreamWaitEvent(v.st, h->advance.ev[0], 0));
        if (launch_advance(h, p, v, ADV_REST, k + 1 < hl_steps)) return -1;
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
  const CadmmStepCfg d;  // the step's defaults, stated once for the handle and the host step
  c->max_iter = d.max_iter;
  c->res_tol = d.res_tol;
  c->use_total_res = d.use_total_res;
  c->rho0 = d.rho0;
  c->tau_incr = d.tau;
  c->rho_max = d.rho_max;
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
  // every row-mode word the rule can give this team (G: by the batch, cadmm_slots) has its k_cadmm instantiation
  if (c.mode == DAT_MODE_CADMM)
    for (int G = 1; G <= 64 / c.n; ++G)
      if (!cadmm_rms_built(cadmm_row_modes(c.n, G))) {
        dat_destroy(h);
        return fail("dat_create: k_cadmm is not built for the row modes of n = " + std::to_string(c.n) + " at " +
                    std::to_string(G) + " scenario slots (DAT_CADMM_RMS, dat_cadmm_lds.hpp)");
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

int dat_control_step(dat_handle* h, const double* state, const double* acc_des, double* f_des, int* iters,
                     int* qp_status, double* min_env_dist, unsigned char* collision, double* err_seq) {
  if (!h) return fail("null handle");
  LoopPlan plan;
  if (step_entry(h, &plan)) return -1;
  const size_t B = h->cfg.batch;
  if (state) HIPCHK(hipMemcpyAsync(h->state, state, sizeof(double) * B * h->S, hipMemcpyHostToDevice, h->stream));
  const Sub u = sub_batch(h, plan);
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
  LoopPlan plan;
  if (step_entry(h, &plan)) return -1;
  const size_t need = (size_t)steps * h->cfg.batch * 6;
  if (need > h->acc_seq_cap) {
    dfree(h, h->acc_seq);
    h->acc_seq_cap = 0;
    if (dalloc(h, &h->acc_seq, need)) return -1;
    h->acc_seq_cap = need;
  }
  HIPCHK(hipMemcpyAsync(h->acc_seq, acc_seq, sizeof(double) * need, hipMemcpyHostToDevice, h->stream));
  Sub u = sub_batch(h, plan);
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
// schedules of the same step chain; which one a call runs is the plan of dat_modes.hpp (loop_plan), made once per
// call (step_entry) and handed to everything below.
//   serial      one sub-batch on the handle's stream; the host waits for each step's control kernels (the rollout
//                still runs while the next step is enqueued).
//   sub-batches  S of them, each on its own stream, no synchronisation between the sub-batches or the steps; the
//                host waits once, for the call's end.
//   overlap      the serial chain with the rollout and the next step's inputs split into two passes
//                over disjoint scenarios: `early` on the advance stream beside the drain's ramp-down, on the
//                scenarios whose done stamp is the step's, started when k_cadmm's class-0 queue has been claimed
//                empty (the host word) or the drain has ended; `rest` on the handle's stream after the drain, on the
//                others.  A scenario's step is the same sequence of the same device functions on the same inputs in
//                either pass.  The inputs of a call's first step are computed for every scenario up front, and none
//                after its last step (the next call starts from the state alone, which dat_set_state may replace).
//   pipeline     (closed_loop_pipelined) the overlap with the next step's drain split likewise: the
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
  // (dat_set_plant and dat_log_begin refuse the pair; this guards a handle put into that state some other way)
  if (h->plant == DAT_PLANT_RP && admit(h, "dat_closed_loop", FEAT_PLANT_RP, feat_bit(FEAT_LOG))) return -1;
  LoopPlan plan;
  if (log_admit(h, hl_steps) || step_entry(h, &plan, std::max(hl_steps, 0))) return -1;
  if (hl_steps > 0) h->env_sub = h->nsub;
  if (plan.schedule == SCHED_PIPELINE ? closed_loop_pipelined(h, plan, hl_steps) : closed_loop_stepped(h, plan, hl_steps))
    return -1;
  if (hl_steps > 0) h->clock += (long long)hl_steps * h->cfg.hl_every;
  return 0;
}

// ---- the tracking law, the clock and the plant ------------------------------------------------------------------
int dat_set_tracking(dat_handle* h, const double* rec, int per_scenario) {
  if (!h) return fail("dat_set_tracking: null handle");
  if (rec && admit(h, "dat_set_tracking", FEAT_TRACKING)) return -1;  // (the law in force is unchanged)
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
  if (plant == DAT_PLANT_RP && admit(h, "dat_set_plant", FEAT_PLANT_RP)) return -1;
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

int dat_debug_row_modes(dat_handle* h, int m0, int m1, int m2) {
  if (!h) return fail("dat_debug_row_modes: null handle");
  if (h->cfg.mode != DAT_MODE_CADMM) return fail("dat_debug_row_modes: C-ADMM handles only");
  if (m0 < 0 && m1 < 0 && m2 < 0) {
    h->force_rms = -1;
    return 0;
  }
  if (m0 < 0 || m0 > 2 || m1 < 0 || m1 > 2 || m2 < 0 || m2 > 2) return fail("dat_debug_row_modes: modes are 0, 1 or 2");
  if (!cadmm_rms_built(rm_pack(m0, m1, m2)))
    return fail("dat_debug_row_modes: k_cadmm is not built for these row modes (DAT_CADMM_RMS)");
  h->force_rms = rm_pack(m0, m1, m2);
  return 0;
}

int dat_debug_tail_rule(dat_handle* h, int tail_prev, int tail_pass) {
  if (!h) return fail("dat_debug_tail_rule: null handle");
  if (h->cfg.mode != DAT_MODE_CADMM) return fail("dat_debug_tail_rule: C-ADMM handles only");
  if (tail_prev < 0 && tail_pass < 0) {
    h->tail_prev = TAIL_PREV;
    h->tail_pass = TAIL_PASS;
    return 0;
  }
  if (tail_prev < 0 || tail_pass < 2) return fail("dat_debug_tail_rule: tail_prev >= 0 and tail_pass >= 2");
  h->tail_prev = tail_prev;
  h->tail_pass = tail_pass;
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

}  // extern "C"
