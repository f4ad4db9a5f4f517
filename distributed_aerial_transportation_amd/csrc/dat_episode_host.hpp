// dat_episode_host.hpp -- the host-side checks of dat_episode_begin / dat_episode_read (include/dat.h): pure functions
// of their arguments, run before anything is copied or launched.  Host code only, no HIP: dat_h_episode.hip includes it, and
// tests/episode_host/ep_check_main.cpp compiles it alone.
#pragma once

#include <climits>
#include <string>

#include "dat_ckpt.hpp"

namespace dat {

// dat_episode_begin's arguments against a handle of (mode, n): the rules, the capacity, then the pool blob (outside
// input: ck_check_header, nothing past `bytes` is read).  *records: the pool's record count.
inline int ep_check_begin(int mode, int n, const dat_episode_rules* rules, const void* blob, long long bytes,
                          int capacity, int* records, std::string* msg) {
  const std::string who = "dat_episode_begin: ";
  if (!rules) return ck_fail(msg, who + "null rules");
  if (capacity < 0) return ck_fail(msg, who + "negative capacity " + std::to_string(capacity));
  if (rules->goal_x != rules->goal_x) return ck_fail(msg, who + "goal_x is NaN (+inf switches the goal off)");
  if (!(rules->bound > 0.0)) return ck_fail(msg, who + "bound must be > 0 (+inf: no bound)");
  if (rules->max_steps < 0) return ck_fail(msg, who + "negative max_steps " + std::to_string(rules->max_steps));
  if (rules->stall_steps < 0) return ck_fail(msg, who + "negative stall_steps " + std::to_string(rules->stall_steps));
  if (rules->stall_steps > 0 && mode == DAT_MODE_CENTRALIZED)
    return ck_fail(msg, who + "the stall rule (stall_steps = " + std::to_string(rules->stall_steps) +
                            ") counts ADMM / DD passes: a centralized handle has none");
  CkHeader h;
  std::string m;
  if (ck_check_header(mode, n, blob, bytes, &h, &m)) return ck_fail(msg, who + "pool: " + m);
  if (h.count < 1) return ck_fail(msg, who + "the pool holds no record");
  if (h.count > INT_MAX) return ck_fail(msg, who + "the pool's record count " + std::to_string(h.count) + " is out of range");
  if (records) *records = (int)h.count;
  return 0;
}

// records [first, first + count) against the `held` of the table
inline int ep_check_read(int first, int count, long long held, std::string* msg) {
  if (first < 0 || count < 0 || (long long)first + count > held)
    return ck_fail(msg, "dat_episode_read: records [" + std::to_string(first) + ", " + std::to_string(first) + " + " +
                            std::to_string(count) + ") must lie in the " + std::to_string(held) + " held");
  return 0;
}

}  // namespace dat
