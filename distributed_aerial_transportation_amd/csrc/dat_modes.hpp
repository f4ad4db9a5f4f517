// dat_modes.hpp -- the two rules of the handle that are pure functions of a few facts, each stated once: which of the
// handle's features exclude which (refusal), and which schedule a dat_closed_loop call runs (loop_plan).  Host code
// only, no HIP: the host units include it (no kernel unit does), and tests/modes_host/modes_check_main.cpp compiles
// it alone and walks every combination of the facts.
#pragma once

#include <string>

#include "../../include/dat.h"

namespace dat {

// ---- which features exclude which --------------------------------------------------------------------------------
// What a handle can hold open (a set: one bit each), and the one action that is refused under one of them.
enum Feature { FEAT_LOG = 0, FEAT_EPISODES, FEAT_TRACKING, FEAT_PLANT_RP, FEAT_COUNT, ACT_CKPT_LOAD = FEAT_COUNT };
constexpr unsigned feat_bit(int m) { return 1u << m; }

// One row per excluding pair, with its reason; a pair of features excludes in either order.  Where several rows
// refuse a call, the first one speaks.
struct Exclusion {
  int a, b;
  const char* reason;
};
constexpr Exclusion EXCLUSIONS[] = {
    {FEAT_LOG, FEAT_EPISODES, "the log does not record episodes yet"},
    {FEAT_LOG, FEAT_PLANT_RP, "the log does not record the rigid-payload plant (DAT_PLANT_RP) yet"},
    {FEAT_EPISODES, FEAT_PLANT_RP, "episodes do not run on the rigid-payload plant (DAT_PLANT_RP) yet"},
    {FEAT_EPISODES, FEAT_TRACKING, "episodes do not run under tracking records yet"},
    {ACT_CKPT_LOAD, FEAT_EPISODES,
     "episodes are open on the handle (a loaded scenario would not be the episode its slot is recorded to run)"},
};
// how the caller closes a feature that is open
constexpr const char* REMEDY[FEAT_COUNT] = {"dat_log_end first", "dat_episode_end first",
                                                    "dat_set_tracking(NULL) first", "dat_set_plant(DAT_PLANT_RQP) first"};

// `caller` wants to open the feature, or do the action, `want` on a handle that holds the set `open`: empty where it
// may, else the message "<caller>: <reason>: <remedy of the open side>".  Nothing has been touched at that point.
inline std::string refusal(const char* caller, int want, unsigned open) {
  for (const Exclusion& x : EXCLUSIONS) {
    const int other = x.a == want ? x.b : x.b == want ? x.a : -1;  // (an action is never the open side)
    if (other >= 0 && other < FEAT_COUNT && (open & feat_bit(other)))
      return std::string(caller) + ": " + x.reason + ": " + REMEDY[other];
  }
  return std::string();
}

// ---- which schedule a dat_closed_loop call runs ------------------------------------------------------------------
// The facts the choice depends on: the handle's configuration and switches, and which of the resources that are
// made on first use (and may fail to be made) are in place.
struct LoopFacts {
  int mode = DAT_MODE_CADMM, nsub = 1;
  bool forest = false, log_open = false, record_err = false;
  bool adv_on = false, pipe_on = false, fused_on = false;
  bool fused_sort_build = false;  // DAT_FUSED_SORT
  bool have_words = false;        // the overlap's stamp arrays, its counters and the mapped host word (dat_create)
  bool have_tail = false, have_advance = false;                    // the tail stream, the advance stream
  bool have_pipe = false, have_lists = false, have_ktabs = false;  // the pipeline's stream, its lists, its key tables
};
enum Schedule { SCHED_SERIAL, SCHED_SUB_BATCHES, SCHED_OVERLAP, SCHED_PIPELINE };
struct LoopPlan {
  Schedule schedule = SCHED_SERIAL;
  bool tail_route = false;  // the tail-routed scenarios' launch beside k_cadmm (else the hand-over inside it)
  bool fused = false;       // an early / rest pass is one k_advance (else the three kernels of the step chain)
  bool fused_sort = false;  // ... and counts the keys of the pipeline's sorts behind it
};

// The overlap and the pipeline run C-ADMM on one sub-batch with no log open (the recording rollout has no passes);
// the pipeline keeps no residual record (its per-step pad is a whole-batch memset).  The concurrent tail launch needs
// a stream of its own beside the step's: with sub-batches a fifth stream would share the hardware queues with them.
// A missing resource steps the schedule down -- pipeline, overlap, serial -- with the same results.
inline LoopPlan loop_plan(const LoopFacts& f) {
  const bool one = f.mode == DAT_MODE_CADMM && f.nsub == 1;
  const bool overlap = f.adv_on && one && !f.log_open && f.have_words && f.have_advance;
  const bool pipeline = f.pipe_on && !f.record_err && overlap && f.have_pipe && f.have_lists && f.have_ktabs;
  LoopPlan p;
  p.schedule = pipeline ? SCHED_PIPELINE : overlap ? SCHED_OVERLAP : f.nsub > 1 ? SCHED_SUB_BATCHES : SCHED_SERIAL;
  p.tail_route = one && f.forest && f.have_tail;
  p.fused = f.fused_on && f.mode == DAT_MODE_CADMM && !f.log_open;
  p.fused_sort = p.fused && f.fused_sort_build && pipeline;
  return p;
}

// the plan if every resource that is made on first use were there: what a call sets out to acquire
inline LoopPlan loop_plan_wanted(LoopFacts f) {
  f.have_tail = f.have_advance = f.have_pipe = f.have_lists = f.have_ktabs = true;
  return loop_plan(f);
}

}  // namespace dat
