// dat_h_episode.hip -- the episodes on the host side (include/dat.h, dat_episode_*): the pool, the outcome table and
// the counters, the kernel arguments the rolling passes take (dat.hip: launch_step_rollout, launch_advance), and the
// reads.  No kernel lives here: the rule runs in k_rollout_agents and k_advance (dat_episode.hpp), and
// dat_episode_begin loads the slots through the checkpoints' scatter kernel.
#include <cmath>

#include "dat_handle.hpp"
#include "dat_episode_host.hpp"

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

namespace {
void ep_free(dat_handle* h) {
  dat_episodes& e = h->ep;
  dfree(h, e.pool);
  dfree(h, e.table);
  dfree(h, e.cnt);
  e = dat_episodes();
}
}  // namespace

extern "C" {

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
  if (admit(h, "dat_episode_begin", FEAT_EPISODES)) return -1;
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
