// dat_h_log.hip -- the closed loop's log on the host side (include/dat.h, dat_log_*): its buffers, the kernel
// arguments the recording rollout takes (dat.hip: launch_step_rollout), the capacity check of a dat_closed_loop call,
// and the reads.  No kernel lives here: k_rollout_agents<true> (dat_k_step.hip) fills the buffers.
#include "dat_handle.hpp"

LogArgs log_args(const dat_handle* h, int off) {
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

extern "C" {

int dat_log_begin(dat_handle* h, const int* scenarios, int count, int log_every, int hl_capacity, int summary) {
  if (!h) return fail("null handle");
  if (h->log.open) return fail("dat_log_begin: a log is already open (dat_log_end first)");
  if (admit(h, "dat_log_begin", FEAT_LOG)) return -1;
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

}  // extern "C"
