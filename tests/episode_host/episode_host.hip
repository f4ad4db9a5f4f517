// Host-side driver of the episode rule (TEST-ONLY): episode_step and episode_record of csrc/dat_episode.hpp, compiled
// with hipcc into tests/episode_host/libdat_episode_host.so and loaded only by tests/.  They are the functions the
// kernels with the episode flag call (episode_lanes, dat_k_step.hip), so the rule can be checked against a numpy
// restatement without a GPU.
#include "../../distributed_aerial_transportation_amd/csrc/dat_episode.hpp"

using namespace dat;

extern "C" {

int eh_acc_ints(void) { return (int)(sizeof(EpAcc) / sizeof(int)); }

// `count` independent cases, each a sequence of `steps` control steps of one episode from fresh accumulators: step t
// of case k sees xl, vl [(k steps + t) x 3], iters, col, mind [k steps + t].  reason [k steps + t]: the rule's verdict
// after that step (the accumulators run on past a verdict, as in an idle slot's arithmetic they would not: the test
// reads every prefix); acc_out [k steps + t]: the accumulators after the step, as (steps, isum, imax, full, run) ints
// and mind_out the smallest distance.
void eh_steps(const dat_episode_rules* rules, int max_iter, int count, int steps, const double* xl, const double* vl,
              const int* iters, const int* col, const double* mind, int* reason, int* acc_out, double* mind_out) {
  for (int k = 0; k < count; ++k) {
    EpAcc c;
    episode_start(c, 0, 0, 0, 0);
    for (int t = 0; t < steps; ++t) {
      const size_t o = (size_t)k * steps + t;
      reason[o] = episode_step(rules[k], max_iter, xl + 3 * o, vl + 3 * o, iters[o], col[o], mind[o], c);
      int* a = acc_out + 5 * o;
      a[0] = c.steps; a[1] = c.isum; a[2] = c.imax; a[3] = c.full; a[4] = c.run;
      mind_out[o] = c.mind;
    }
  }
}

// record and idle flag of slot s[k]'s j[k]-th episode
void eh_records(const int* s, const int* j, int count, int B, int P, int wrap, int* record, int* idle) {
  for (int k = 0; k < count; ++k) record[k] = episode_record(s[k], j[k], B, P, wrap, idle + k);
}

}  // extern "C"
