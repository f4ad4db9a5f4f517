// dat_episode.hpp -- when a scenario's episode ends and which pool record its slot takes next (dat_episode_*,
// include/dat.h), stated once for the kernels (rollout_lanes<., ., true>: k_rollout_agents and k_advance with the
// episode flag, dat_k_step.hip) and the host (tests/episode_host).  Pure functions of their arguments: the early pass
// of the overlapped schedules and the rest pass that follows it evaluate the same function on the same inputs and
// come to the same verdict.
//
// A scenario's accumulators (EpAcc, one per scenario: KArgs::epacc, an array of the handle's table) are updated once
// per control step, by episode_step, which then names the reason the episode ends for (DAT_EP_*, dat_layout.h; the
// lowest code that fires wins) or DAT_EP_NONE.
#pragma once

#include "../../include/dat.h"
#include "dat_core.hpp"

namespace dat {

struct EpAcc {
  double mind;      // smallest min_env_dist of the episode's steps (+inf: none yet)
  long long start;  // tick of the episode's first control step
  int steps;        // control steps computed
  int isum, imax;   // sum and maximum of iters
  int full;         // steps at max_iter + 1 passes
  int run;          // ... the current run of them
  int episodes;     // episodes this slot has finished
  int record;       // the pool record the running episode started from
  int idle;         // the pool is used up (wrap = 0): the slot runs on and ends no more
};
static_assert(sizeof(EpAcc) == 48, "EpAcc: six 8-byte words");

DAT_HD bool ep_finite(double x) { return x - x == 0.0; }

// the accumulators of an episode that starts from pool record `record` with its first control step at tick `start`
DAT_HD void episode_start(EpAcc& c, int record, long long start, int episodes, int idle) {
  c.mind = HUGE_VAL;
  c.start = start;
  c.steps = c.isum = c.imax = c.full = c.run = 0;
  c.episodes = episodes;
  c.record = record;
  c.idle = idle;
}

// One control step of the episode: the step's published outputs (iters, col, mind) go into the accumulators, then the
// rule is evaluated on them and the pre-rollout xl, vl.  Returns the reason, DAT_EP_NONE: the episode goes on.
DAT_HD int episode_step(const dat_episode_rules& r, int max_iter, const double* xl, const double* vl, int iters,
                        int col, double mind, EpAcc& c) {
  const bool full = iters > max_iter;
  c.steps += 1;
  c.isum += iters;
  c.imax = iters > c.imax ? iters : c.imax;
  c.full += full ? 1 : 0;
  c.run = full ? c.run + 1 : 0;
  if (mind < c.mind) c.mind = mind;
  bool bad = false;
  double m = 0.0;
  for (int k = 0; k < 3; ++k) {
    bad = bad || !ep_finite(xl[k]) || !ep_finite(vl[k]);
    const double ax = fabs(xl[k]);
    if (ax > m) m = ax;
  }
  if (bad || m > r.bound) return DAT_EP_DIVERGED;
  if (r.on_collision && col) return DAT_EP_COLLISION;
  if (xl[0] >= r.goal_x) return DAT_EP_GOAL;
  if (r.stall_steps > 0 && c.run >= r.stall_steps) return DAT_EP_STALL;
  if (r.max_steps > 0 && c.steps >= r.max_steps) return DAT_EP_TIME_LIMIT;
  return DAT_EP_NONE;
}

// The pool record slot s (its index in the whole batch of B) starts its j-th episode from, j >= 0, in a pool of P:
// (s + j B) mod P.  With wrap = 0 an index s + j B that reaches P gives s mod P and *idle = 1.
DAT_HD int episode_record(int s, int j, int B, int P, int wrap, int* idle) {
  const long long idx = (long long)s + (long long)j * B;
  if (!wrap && idx >= P) {
    *idle = 1;
    return s % P;
  }
  *idle = 0;
  return (int)(idx % P);
}

}  // namespace dat
