// dat_k_step.hip -- the kernels of a step around the drains: the rollout / advance family (k_env_class<*>, k_bucket,
// k_bucket_adv<*>, k_bucket_scatter<*>, k_rollout_agents<*, *, *>, k_desired<*>, k_advance<*, *>, k_low_level), and with
// them k_warm, k_env, the rigid-payload, PMRL and checkpoint kernels.  The family is one unit: its kernels share
// device functions (ll_control_agent, rollout_lanes, env_class_lanes) for which the inliner's choices depend on the
// callers the unit holds (the comment at k_low_level), so a kernel compiled without its siblings comes out different.
// (dat_launch.hpp: the units.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>

#include "dat_dd_step.hpp"
#include "dat_launch.hpp"
#include "dat_pmrl_step.hpp"

using namespace dat;

namespace {

// env class of one agent QP: 0 if it carries no env row, otherwise the smallest class whose slots
// hold the rows set_env_rows keeps (nonzero rows, compacted).  An all-zero row with a positive
// right-hand side (0 >= rhs > 0: the reference's QP is infeasible, set_env_rows flags it) also
// needs an env class.
__device__ inline int env_class_of(unsigned emask, const double lhs[DAT_NENV][3], const double rhs[DAT_NENV]) {
  bool need = false;
  int k = 0;
#pragma unroll
  for (int j = 0; j < DAT_NENV; ++j) {
    const bool on = (emask >> j) & 1u;
    const bool zero = lhs[j][0] == 0.0 && lhs[j][1] == 0.0 && lhs[j][2] == 0.0;
    need = need || (on && (!zero || rhs[j] > 0.0));
    k += (on && !zero) ? 1 : 0;
  }
  if (!need) return 0;
  int c = 1;
  while (c < NCLS - 1 && k > class_env_rows(c)) ++c;
  return c;
}

// Env rows of the n agents of each scenario of a 64-lane block, computed cooperatively
// (control/rqp_cadmm.py:307-373 from env_rows' pieces, dat_core.hpp).  The payload capsule and the x-window of
// candidate trees are the same for every agent of a scenario; only the camera-cone filter differs
// (cos 100 deg: most agents see most trees).  Lane i of a scenario evaluates trees base + i of each
// chunk of n candidates -- range test, capsule_tree distance and the CBF row, once per tree instead
// of once per agent that sees it -- and publishes them in LDS; then every lane runs its own cone
// filter and sorted insertion over the chunk in tree order.  The pieces and the insertion order are env_rows',
// so the rows are bitwise identical by construction (test_gpu_env_rows_reference.py checks it).
// Must be called by every lane of the block (barriers inside).
constexpr int ENV_CE = 8;  // published entry: in range, c.x, c.y, dd, l3[3], r1
// LDS stride of a published entry: 9 doubles (18 dwords), so the 32 lanes of a ds_*_b64 half-wave
// start on 32 distinct even banks (a stride of 8 doubles put 64 lanes on 4 bank pairs: 16-way conflicts)
constexpr int ENV_CS = ENV_CE + 1;
__device__ EnvOut env_rows_coop(const double* prm, int n, const double* st, const double* trees, int ntree, int i,
                                int ls, bool valid, double alpha_env, unsigned* mask, double lhs[DAT_NENV][3],
                                double rhs[DAT_NENV], double* ent /* LDS: 64 x ENV_CS */) {
  EnvOut out;
  out.collision = 0;
  out.min_env_dist = valid ? prm[DAT_P_VISR] : 0.0;
  *mask = 0u;
  const bool any = valid && trees != nullptr && ntree > 0;
  bool dead = !any;  // this agent keeps no row (it still evaluates its share of the trees)
  EnvFrame fr;
  EnvCam cam;
  int t0 = 0;
  if (any) {
    env_frame(prm, n, st, fr);
    if (!env_camera(prm, n, st, i, cam)) {
      out.collision = 1;
      dead = true;
    }
    t0 = env_window_begin(fr, trees, ntree);
  }
  EnvSeen seen;
  env_clear(seen, lhs, rhs);
  double* mine = ent + (size_t)threadIdx.x * ENV_CS;
  const double* grp = ent + (size_t)(ls * n) * ENV_CS;
  for (int base = t0;; base += n) {
    // this lane's tree of the chunk
    const int t = base + i;
    const bool cand = any && t < ntree && trees[3 * t] <= fr.ctr[0] + fr.reach;
    double e[ENV_CE] = {0, 0, 0, 1e300, 0, 0, 0, 0};
    if (cand) {
      const double* c = trees + 3 * t;
      if (env_in_range(fr, c)) {
        e[0] = 1.0; e[1] = c[0]; e[2] = c[1];
        e[3] = env_tree_row(fr, alpha_env, c, e + 4);
      }
    }
    // every lane of the block takes part in the barriers; the loop ends when no lane had a candidate
    if (!__syncthreads_or(cand)) break;
#pragma unroll
    for (int k = 0; k < ENV_CE; ++k) mine[k] = e[k];
    __syncthreads();
    if (!dead) {
      for (int j = 0; j < n; ++j) {  // the chunk in tree order
        const double* q = grp + (size_t)j * ENV_CS;
        if (q[0] == 0.0) continue;
        if (!env_in_cone(cam, q[1], q[2])) continue;
        const double dd = q[3];
        if (dd < ENV_TOUCH) out.collision = 1;
        env_see(seen, dd, q + 4, lhs, rhs);
      }
    }
    __syncthreads();  // the chunk is consumed before the next one is published
  }
  if (!dead && seen.cnt > 0 && fr.speed > 0.0) {
    out.min_env_dist = seen.dmin;
    *mask = env_mask(seen);
  }
  return out;
}

// The body of k_env_class for the lanes of one block (lane ls * n + i: agent i of scenario sc; valid: the scenario
// takes part), stated once for k_env_class and k_advance.  Every lane of the block must call it (barriers inside).
// nd, cl, md: 64 words of LDS each; ent: 64 x ENV_CS doubles.  lhs, rhs: the lane's sorted row slots, the
// kernel's own arrays: declared here they would be optimised once with this function and again with the kernel
// it is inlined into, and come out wholly scalarised, past the register bound (k_env_class: 180 B/lane of scratch
// against 88 before the body was factored out; as the kernel's, none at 230 VGPRs).
template <int ADV>
__device__ __forceinline__ void env_class_lanes(const KArgs& a, int n, int lane, int ls, int i, int sc, bool valid,
                                                int* nd, int* cl, double* md, double* ent, double lhs[DAT_NENV][3],
                                                double rhs[DAT_NENV]) {
  int need = 0, col = 0;
  double dist = 1e300;
  const double* prm = valid ? prm_of(a, sc) : a.params;
  const double* trees = nullptr;
  int nt = 0;
  if (valid) forest_of(a, sc, &trees, &nt);
  unsigned emask;
  EnvOut e = env_rows_coop(prm, n, valid ? a.state + (size_t)sc * a.S : nullptr, trees, nt, i, ls, valid,
                           prm[DAT_P_AENVD], &emask, lhs, rhs, ent);
  if (valid) {
    need = env_class_of(emask, lhs, rhs);
    col = e.collision;
    dist = e.min_env_dist;
    // hand the rows to k_cadmm (lanes hold consecutive agents: every store is coalesced)
    const size_t NA = (size_t)a.B * n, g = (size_t)sc * n + i;
    a.emask[g] = emask;
#pragma unroll
    for (int j = 0; j < DAT_NENV; ++j) {
      if (!((emask >> j) & 1u)) continue;  // only the slots the mask marks are read back
      a.erows[(4 * j + 0) * NA + g] = lhs[j][0];
      a.erows[(4 * j + 1) * NA + g] = lhs[j][1];
      a.erows[(4 * j + 2) * NA + g] = lhs[j][2];
      a.erows[(4 * j + 3) * NA + g] = rhs[j];
    }
  }
  nd[lane] = need;
  cl[lane] = col;
  md[lane] = dist;
  __syncthreads();
  int cnum = 0;
  double cmin = 1e300;
  if (valid && i == 0) {
    int cls = 0, c = 0;
    double m = prm_of(a, sc)[DAT_P_VISR];
    for (int k = 0; k < n; ++k) {
      cls = max(cls, nd[ls * n + k]);
      c |= cl[ls * n + k];
      m = fmin(m, md[ls * n + k]);
    }
    // previous step's ADMM iterations, then its slowest agent QP's IPM iterations: within a class the
    // longest scenarios are claimed first and scenarios sharing a wavefront tend to need similar
    // numbers of ADMM passes and of IPM iterations per pass (a pass lasts as long as its slowest lane)
    // (beside the running drain the two come as the drain published them: write-through, read past the caches)
    const int pit = ADV == ADV_EARLY ? ld_wt(a.iters + sc) : a.iters[sc];
    const int pmx = ADV == ADV_EARLY ? ld_wt(a.ipmx + sc) : a.ipmx[sc];
    const int bin = NPB * iter_bin(pit) + ipm_bin(pmx);
    // a scenario wedged in a stall (previous step > TAIL_PREV passes) goes to the tail (key NKEY + class); with
    // sub-batches it stays in k_cadmm's queue, which hands it over after its first pass (the tail rule), the
    // same arithmetic
    a.need[sc] = a.route && tail_wedged(pit, a.tail_prev) ? NKEY + cls : cls * NIB + (NIB - 1 - bin);
    a.col[sc] = (unsigned char)c;
    a.mind[sc] = m;
    cnum = c;
    cmin = m;
  }
  // collisions and the smallest env distance of the step (bench stats; one atomic per wavefront, the minimum only
  // when it undercuts the running one)
  for (int off = 32; off > 0; off >>= 1) {
    cnum += __shfl_xor(cnum, off);
    cmin = fmin(cmin, __shfl_xor(cmin, off));
  }
  if (lane == 0) {
    if (cnum) atomicAdd(a.counters + CNT_COLL, (unsigned long long)cnum);
    // (an order-preserving key of the signed distance: a collided payload's distance is negative)
    unsigned long long* pm = a.counters + CNT_COLL + 1;
    const unsigned long long key = dist_key(cmin);
    if (cmin == cmin && key < *(volatile unsigned long long*)pm) atomicMin(pm, key);
  }
}
// Two wavefronts per SIMD (256 VGPRs at most): the build without the bound (290 registers, no scratch, one wavefront
// per SIMD) measured slower, C4 A/B 3.58 / 3.61 -> 3.70 / 3.80 ms per step (round 4).  Three or four wavefronts
// per SIMD (168 / 128 VGPRs, the sorted row slots spilled) measured 3.2-3.6x slower by kernel trace: 0.24 ->
// 0.77 / 0.87 ms (round 4).
// ADV (dat_kargs.hpp): the scenarios that take part; a scenario's lanes do together or not at all, the others are
// carried through the barriers like the lanes past the batch.  ADV_ALL compiles to the kernel without a gate.
template <int ADV>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_env_class(KArgs a) {
  __shared__ int nd[64], cl[64];
  __shared__ double md[64];
  __shared__ double ent[64 * ENV_CS];
  const int n = a.n, G = 64 / n, NT = G * n;
  const int lane = threadIdx.x;
  const int ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  const bool valid = (lane < NT) && (sc < a.B) && adv_gate<ADV, false>(a, sc);
  if constexpr (ADV != ADV_ALL)
    if (!__syncthreads_or(valid)) return;  // no scenario of the block takes part
  double lhs[DAT_NENV][3], rhs[DAT_NENV];
  env_class_lanes<ADV>(a, n, lane, ls, i, sc, valid, nd, cl, md, ent, lhs, rhs);
}

// Counting sort of the scenario ids by key (need[] in [0, NKEY)): list holds the ids of key 0, then
// key 1, ...; count is the class table (ScountRow, dat_kargs.hpp): size / start of env class c (keys c NIB ..
// c NIB + NIB - 1), its queue heads zeroed.  Within a class the key is the previous step's (ADMM
// iterations, slowest agent's IPM iterations) bin, in decreasing order, so the longest scenarios are
// claimed first.  One BUCKET_T-thread workgroup, coalesced strided reads, LDS atomics for the
// histogram and the scatter cursors: the order within a key is not fixed, which only changes which
// scenarios share a wavefront, never a scenario's arithmetic (the capped-grid test compares two
// different groupings bitwise).
constexpr int BUCKET_T = 1024;
static_assert(NKEY_ALL <= BUCKET_T, "bucket_sort initialises one key per thread");
// ADV_EARLY / ADV_REST: ... of the scenarios whose early-rollout mark adv[] is / is not `serial`: the step
// pipeline's two drains of a step take disjoint lists.  A tail-routed scenario (key >= NKEY) goes to the ADV_REST
// list wherever it was advanced, so that a step's routed scenarios run in one tail launch: the tail launches of the
// two drains share a stream, and two of them holding stalled scenarios run one after the other.  need[] of a
// scenario the early pass left out may be stale (its env rows are not computed yet) and is not read by the ADV_EARLY
// sort.  ADV_ALL: every scenario (adv is not read).
// Does the sort of mode ADV list scenario q?
template <int ADV>
__device__ __forceinline__ bool sort_takes(int q, const int* need, const int* adv, int serial) {
  if constexpr (ADV == ADV_ALL) return true;
  else return (adv[q] == serial && need[q] < NKEY) == (ADV == ADV_EARLY);
}
// The class table of a sorted list from its keys' sizes and starts (one thread)
__device__ __forceinline__ void class_table(int* count, const int* tot, const int* kstart) {
  int st = 0;
  for (int cl = 0; cl < NCLS; ++cl) {
    int sz = 0;
    for (int b = 0; b < NIB; ++b) sz += tot[cl * NIB + b];
    count[sc_at(SC_SIZE, cl)] = sz;
    count[sc_at(SC_START, cl)] = st;
    count[sc_at(SC_HEAD, cl)] = 0;       // queue head of the class (k_cadmm)
    count[sc_at(SC_HAND_SIZE, cl)] = 0;  // hand-over list of the class (k_cadmm -> k_cadmm_tail) and its head
    count[sc_at(SC_HAND_HEAD, cl)] = 0;
    st += sz;
  }
  for (int cl = 0; cl < NCLS; ++cl) {  // the tail-routed stretches (keys NKEY + class) behind them
    count[sc_at(SC_TAIL_SIZE, cl)] = tot[NKEY + cl];
    count[sc_at(SC_TAIL_START, cl)] = kstart[NKEY + cl];
    count[sc_at(SC_TAIL_HEAD, cl)] = 0;
  }
}
__device__ __forceinline__ int sort_key(int need) { return min(max(need, 0), NKEY_ALL - 1); }
template <int ADV>
__device__ __forceinline__ void bucket_sort(int B, const int* need, int* list, int* count, const int* adv,
                                            int serial) {
  const auto take = [&](int q) { return sort_takes<ADV>(q, need, adv, serial); };
  __shared__ int hist[NKEY_ALL], kstart[NKEY_ALL], cursor[NKEY_ALL], tot[NKEY_ALL];
  const int t = threadIdx.x;
  if (t < NKEY_ALL) { hist[t] = 0; cursor[t] = 0; }
  __syncthreads();
  for (int q = t; q < B; q += BUCKET_T)
    if (take(q)) atomicAdd(&hist[sort_key(need[q])], 1);
  __syncthreads();
  if (t == 0) {
    int st = 0;
    for (int k = 0; k < NKEY_ALL; ++k) { kstart[k] = st; tot[k] = hist[k]; st += hist[k]; }
  }
  __syncthreads();
  for (int q = t; q < B; q += BUCKET_T) {
    if (!take(q)) continue;
    const int key = sort_key(need[q]);
    list[kstart[key] + atomicAdd(&cursor[key], 1)] = q;
  }
  if (t == 0) class_table(count, tot, kstart);
}
__global__ __launch_bounds__(BUCKET_T) void k_bucket(int B, const int* need, int* list, int* count) {
  bucket_sort<ADV_ALL>(B, need, list, count, nullptr, 0);
}
template <int ADV>
__global__ __launch_bounds__(BUCKET_T) void k_bucket_adv(int B, const int* need, int* list, int* count,
                                                         const int* adv, int serial) {
  static_assert(ADV == ADV_EARLY || ADV == ADV_REST, "the unfiltered sort is k_bucket");
  bucket_sort<ADV>(B, need, list, count, adv, serial);
}

// The filtered sort behind k_advance, which has counted the keys where it made them: a key table (KeyTab) holds the
// histogram of exactly the scenarios sort_takes<ADV> lists -- the early k_advance counts a scenario with a key below
// NKEY into the main drain's table and a tail-routed one into the rest drain's, the late one everything into the
// rest drain's -- so the sort is the scatter alone, over SCATTER_T scenarios per block.  Every block derives the key
// starts from the counts (first wavefront, three keys per lane); a block ranks its scenarios within their keys in
// LDS and claims a stretch per key it holds with one cursor atomic (the order within a key is not fixed, as in
// bucket_sort); block 0 writes the class table.  (A claim per wavefront and key, one after the other, left the
// 65,536-scenario sort at the single workgroup's 66 us: 1,024 wavefronts' claims queue on the few keys most
// scenarios share.)
// The tables alternate (two per drain kind): the last block zeroes `other`, the table of the same kind whose
// previous reader ended before this kernel started and whose next k_advance starts after it has ended
// (closed_loop_pipelined), so no launch waits for a zeroed table.
constexpr int SCATTER_T = 256;
static_assert(NKEY_ALL <= 3 * 64, "k_bucket_scatter scans three keys per lane of one wavefront");
static_assert(NKEY_ALL <= SCATTER_T, "k_bucket_scatter claims one key per thread");
template <int ADV>
__global__ __launch_bounds__(SCATTER_T) void k_bucket_scatter(int B, const int* need, int* list, int* count,
                                                              const int* adv, int serial, int* tab, int* other) {
  static_assert(ADV == ADV_EARLY || ADV == ADV_REST, "the unfiltered sort is k_bucket");
  __shared__ int kstart[NKEY_ALL], tot[NKEY_ALL], hist[NKEY_ALL], base[NKEY_ALL];
  const int t = threadIdx.x;
  if (t < NKEY_ALL) hist[t] = 0;
  if (t < 64) {  // exclusive prefix sum of the counts
    int c[3], s = 0;
    for (int j = 0; j < 3; ++j) {
      const int k = 3 * t + j;
      c[j] = k < NKEY_ALL ? tab[KT_COUNT + k] : 0;
      s += c[j];
    }
    int incl = s;
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off);
      if (t >= off) incl += v;
    }
    int st = incl - s;
    for (int j = 0; j < 3; ++j) {
      const int k = 3 * t + j;
      if (k < NKEY_ALL) { kstart[k] = st; tot[k] = c[j]; }
      st += c[j];
    }
  }
  __syncthreads();
  const int q = blockIdx.x * SCATTER_T + t;
  const bool take = q < B && sort_takes<ADV>(q, need, adv, serial);
  const int key = take ? sort_key(need[q]) : -1;
  // the block's rank within its key (LDS), then one claim per key the block holds, all keys' claims in flight together
  const int rank = take ? atomicAdd(&hist[key], 1) : 0;
  __syncthreads();
  if (t < NKEY_ALL && hist[t]) base[t] = atomicAdd(tab + KT_CURSOR + t, hist[t]);
  __syncthreads();
  const int pos = take ? kstart[key] + base[key] + rank : -1;
  if ((unsigned)pos < (unsigned)B) list[pos] = q;  // (within the list whatever the tables hold)
  if (blockIdx.x == 0 && t == 0) class_table(count, tot, kstart);
  if (blockIdx.x == gridDim.x - 1)
    for (int k = t; k < KT_INTS; k += SCATTER_T) other[k] = 0;
}

// ------------------------------------------------------------------------------------------------
// rollout / desired acceleration / warm start
// ------------------------------------------------------------------------------------------------
// `steps` simulation steps (sim_step, system/rigid_quadrotor_payload.py:129-222) with one lane per (scenario, agent): G = floor(64/n) scenarios
// per 64-lane block.  Lane i runs agent i's low-level law, rotational dynamics and attitude
// integration; the payload's force / moment sums go through LDS and every lane of the scenario
// integrates the payload identically (sums in agent order, the pieces of sim_step, dat_core.hpp: bitwise
// the same trajectory by construction).  Per-lane state is one quadrotor plus the payload (~40 doubles), so nothing
// spills and the kernel runs many wavefronts per SIMD, for any n (k_rollout<0> kept the whole state
// of a large team in scratch).
//
// LOG = true (a log is open, dat_log_begin): the launch is one HL period of dat_closed_loop and also writes the
// period's records (layouts: dat_layout.h DAT_LOG_*).  On entry lane i of a recorded scenario writes its f_des
// and qp_status, lane 0 the rest of the HL record from the entry state (the HL instant's); lane 0 of every
// scenario writes the summary tier.  At a logged step lane i writes the thrust and moment it applies and, after
// the integration (and the polar projection), its R and w; lane 0 the payload and the tracking errors.  A
// scenario's record is contiguous and a lane's stores are runs of 4, 9 + 3 and 20 doubles, like the state
// write-back below.  LOG = false compiles to the kernel without any of it.
constexpr int RO_X = 6;  // per lane in LDS: u = f R e3 (3), hat(r_com) Rl' u (3)
constexpr double REF_X_OFFSET = 1.5;  // x_ref leads the payload by 1.5 m (example/rqp_example.py:36)
// the mountain record m of scenario sc's desired-acceleration law (without a forest: the flat default)
__device__ inline void mountain_of(const KArgs& a, int sc, double* m) {
  const int f = (a.nforest > 0) ? (a.scen_forest ? a.scen_forest[sc] : 0) : -1;
  if (f < 0 || a.mountain == nullptr) {
    m[DAT_M_CX] = 30.0; m[DAT_M_CY] = 0.0; m[DAT_M_RADIUS] = 25.0; m[DAT_M_SPHERE_R] = 1e300; m[DAT_M_DEPTH] = 0.0;
  } else {
    for (int k = 0; k < DAT_MOUNTAIN_SIZE; ++k) m[k] = a.mountain[(size_t)f * DAT_MOUNTAIN_SIZE + k];
  }
}
// ---- episodes (dat_episode_*; the rule: dat_episode.hpp) -------------------------------------------------------------
// the array and the word in it behind word x of scenario s's checkpoint record (null: an int word or padding)
__device__ __forceinline__ double* ep_word(const dat::CkArgs& c, int s, int x) {
  for (int k = 0; k < c.nf; ++k) {
    const int d = x - c.off[k];
    if ((unsigned)d < (unsigned)c.w[k]) return c.f[k] + (size_t)s * c.w[k] + d;
  }
  return nullptr;
}
// The episode step of the scenarios of one block, between their control step and their rollout, for the lanes that
// take part in the pass (valid; lane ls * n + i: agent i of scenario sc of the launch, off + sc of the batch).  The
// scenario's first lane updates a copy of the accumulators and evaluates the rule on the state in memory and the
// step's published outputs; the verdict goes to the scenario's lanes.
//   The episode goes on: the accumulators are stored, the pass rolls the scenario out.
//   It ends, ADV_EARLY: nothing is stored and the scenario leaves the pass (*valid = false): unmarked, it is the rest
//     pass's, which runs after every drain of the step has ended and comes to the same verdict from the same inputs.
//     (The drain that finished the scenario stores its warm state with plain stores and may still be running on
//     other CUs: a respawn here would race with lines not yet written back.  DESIGN.md 3.)
//   It ends, otherwise: the first lane appends the outcome and starts the accumulators of the slot's next episode;
//     the scenario's lanes copy the pool record over the scenario's arrays, each word to the place k_ckpt_scatter
//     gives it.  done[] and adv[] stay as the pass leaves them for a scenario it advanced.  Returns true: the pass does
//     not roll the scenario out (its next inputs come from the new state, like any scenario's of the pass).
// An idle slot (wrap = 0, the pool used up) is rolled out like a scenario of the plain loop.
// Every lane of the wavefront must call it (shuffles inside).
template <int ADV>
__device__ __forceinline__ bool episode_lanes(const KArgs& a, const EpArgs& ep, int n, int ls, int i, int sc,
                                              bool* valid) {
  int reason = DAT_EP_NONE;
  if (*valid && i == 0) {
    EpAcc c = a.epacc[sc];
    if (!c.idle) {
      const double* st = a.state + (size_t)sc * a.S;
      double xl[3], vl[3];
      for (int k = 0; k < 3; ++k) {
        xl[k] = st[DAT_S_XL(n) + k];
        vl[k] = st[DAT_S_VL(n) + k];
      }
      // (beside the running drain iters comes as the drain published it: write-through, read past the caches;
      // col and mind were written ahead of the drain)
      const int it = ADV == ADV_EARLY ? ld_wt(a.iters + sc) : a.iters[sc];
      reason = episode_step(ep.rules, a.max_iter, xl, vl, it, a.col[sc], a.mind[sc], c);
      if (reason == DAT_EP_NONE) {
        a.epacc[sc] = c;
      } else if (ADV == ADV_EARLY) {
        atomicAdd(ep.cnt + EPC_DEFERRED, 1ull);
      } else {
        const int s = ep.off + sc;
        atomicAdd(ep.cnt + EPC_ENDED + reason, 1ull);
        atomicAdd(ep.cnt + EPC_RESPAWN + 1, 1ull);
        const unsigned long long at = atomicAdd(ep.cnt + EPC_COUNT, 1ull);
        if (at < (unsigned long long)ep.cap) {
          double* r = ep.table + (size_t)at * DAT_EP_WORDS;
          r[DAT_EP_SLOT] = __hiloint2double(c.episodes, s);
          r[DAT_EP_RECORD] = __hiloint2double(reason, c.record);
          r[DAT_EP_START] = __longlong_as_double(c.start);
          r[DAT_EP_END] = __longlong_as_double(ep.tick);
          r[DAT_EP_STEPS] = __hiloint2double(c.isum, c.steps);
          r[DAT_EP_ITMAX] = __hiloint2double(c.full, c.imax);
          r[DAT_EP_RUN] = __hiloint2double(0, c.run);
          r[DAT_EP_MIND] = c.mind;
          for (int k = 0; k < 3; ++k) {
            r[DAT_EP_XL + k] = xl[k];
            r[DAT_EP_VL + k] = vl[k];
          }
        } else {
          atomicAdd(ep.cnt + EPC_LOST, 1ull);
        }
        int idle;
        const int rec = episode_record(s, c.episodes + 1, ep.batch, ep.P, ep.rules.wrap, &idle);
        if (idle) atomicAdd(ep.cnt + EPC_IDLE, 1ull);
        EpAcc nx;
        episode_start(nx, rec, ep.tick + ep.hl_every, c.episodes + 1, idle);
        a.epacc[sc] = nx;
        reason = -1 - rec;  // to the scenario's lanes: respawn from record rec
      }
    }
  }
  reason = __shfl(reason, (ls * n) & 63);
  if (!*valid || reason == DAT_EP_NONE) return false;
  if constexpr (ADV == ADV_EARLY) {
    *valid = false;
    return false;
  } else {
    const dat::CkArgs& c = ep.ck;
    const int s = ep.off + sc;
    const double* rec = ep.pool + (size_t)(-1 - reason) * c.words;
    for (int x = i; x < c.words; x += n) {
      const double v = rec[x];
      if ((unsigned)(x - c.ints_off) < (unsigned)CK_INT_WORDS) {
        const int i0 = 2 * (x - c.ints_off);
        if (c.ints[i0]) c.ints[i0][s] = __double2loint(v);
        if (c.ints[i0 + 1]) c.ints[i0 + 1][s] = __double2hiint(v);
      } else if (double* p = ep_word(c, s, x)) {
        *p = v;
      }
    }
    return true;
  }
}

// ADV (dat_kargs.hpp): the scenarios that take part.  The early pass runs beside the drain on the scenarios whose
// done stamp is this step's and reads their f_des as the drain published it (write-through, past the caches); it
// marks them in adv, and both passes count their scenarios (advcnt).  ADV_ALL compiles to the kernel without a gate.
// EP: episodes are open (dat_episode_begin): a scenario's episode step stands between the gate and the rollout
// (episode_lanes); a respawned scenario takes part in the pass and is not rolled out.  EP = false compiles to the
// kernel without any of it.
// The body of k_rollout_agents for the lanes of one block, stated once for k_rollout_agents and k_advance: the gate
// and its count, the steps, the write-back and the adv[] mark.  xs: 64 x RO_X doubles of LDS.  Returns false when no
// scenario of the block takes part (nothing was done: the kernel returns); *took_part: this lane's scenario took part.
template <bool LOG, int ADV, bool EP = false>
__device__ __forceinline__ bool rollout_lanes(const KArgs& a, int steps, double dt, const double* fdes,
                                              const std::conditional_t<LOG, LogArgs, NoLog>& lg, double* xs,
                                              bool* took_part, const std::conditional_t<EP, EpArgs, NoEp>& ep = {}) {
  static_assert(!LOG || ADV == ADV_ALL, "the logging rollout is not gated");
  static_assert(!LOG || !EP, "the logging rollout knows no episodes");
  const int n = a.n, G = 64 / n, NT = G * n;
  const int lane = threadIdx.x, ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  bool valid = lane < NT && sc < a.B;
  [[maybe_unused]] bool roll = true;  // EP: false where the scenario was respawned instead
  if constexpr (ADV != ADV_ALL) {
    // (a scenario's lanes follow its first lane's reading of the stamp)
    valid = __shfl((int)(valid && adv_gate<ADV, true>(a, sc)), (ls * n) & 63) != 0 && valid;
    // (the stamp is read before the bytes it covers: the loads below are issued after this branch)
    asm volatile("" ::: "memory");
    if constexpr (EP) roll = !episode_lanes<ADV>(a, ep, n, ls, i, sc, &valid);
    const unsigned long long took = __ballot(valid && i == 0);
    if (!took) return false;  // no scenario of the block takes part (one wavefront: uniform)
    if (lane == 0) atomicAdd(a.advcnt + (ADV == ADV_EARLY ? 0 : 1), (unsigned long long)__builtin_popcountll(took));
  } else if constexpr (EP) {
    roll = !episode_lanes<ADV>(a, ep, n, ls, i, sc, &valid);
  }
  *took_part = valid;
  if constexpr (EP) valid = valid && roll;  // from here on: the scenarios the pass rolls out
  const double* prm = valid ? prm_of(a, sc) : a.params;
  double* g = valid ? a.state + (size_t)sc * a.S : nullptr;
  double R[9], W[3], xl[3], vl[3], Rl[9], wl[3], fd[3];
  int cnt = 0;
  if (valid) {
    for (int k = 0; k < 9; ++k) { R[k] = g[DAT_S_R(n) + 9 * i + k]; Rl[k] = g[DAT_S_RL(n) + k]; }
    for (int c = 0; c < 3; ++c) {
      W[c] = g[DAT_S_W(n) + 3 * i + c];
      xl[c] = g[DAT_S_XL(n) + c];
      vl[c] = g[DAT_S_VL(n) + c];
      wl[c] = g[DAT_S_WL(n) + c];
      fd[c] = ADV == ADV_EARLY ? ld_wt(fdes + (size_t)sc * 3 * n + 3 * i + c) : fdes[(size_t)sc * 3 * n + 3 * i + c];
    }
    cnt = a.counter[sc];
  }
  // LOG: what a lane needs again at a logged step waits in LDS (its slot; lane 0 of a scenario: x_ref, v_ref of
  // this HL period), each word read back by the lane that wrote it (no barrier needed), so the step loop carries no
  // per-lane log state of its own; the next logged step of the launch and its record are the same for every lane
  __shared__ int lslot[LOG ? 64 : 1];
  __shared__ double lref[LOG ? 64 / 3 * 6 : 1];
  [[maybe_unused]] int lnext = 0;
  [[maybe_unused]] double* lrec = nullptr;  // slot 0 of the record of that step
  if constexpr (LOG) {
    const long long first = (lg.clock + lg.log_every - 1) / lg.log_every;  // first logged step / log_every
    lnext = (int)(first * lg.log_every - lg.clock);
    lrec = lg.step + (size_t)(first - lg.step_base) * lg.nslot * DAT_LOG_ST_WORDS(n);
    int slot = -1;
    if (valid) {
      const long long hk = lg.clock / lg.hl_every - lg.hl_base;
      if (i == 0 && lg.sum_iters) {
        const size_t o = (size_t)hk * lg.batch + sc;
        lg.sum_iters[o] = a.iters[sc];
        lg.sum_mind[o] = a.mind[sc];
        lg.sum_col[o] = a.col[sc];
      }
      slot = lg.slot[sc];
      if (slot >= 0) {
        double* r = lg.hl + ((size_t)hk * lg.nslot + slot) * DAT_LOG_HL_WORDS(n);
        int* ri = reinterpret_cast<int*>(r + DAT_LOG_HL_INTS(n));
        for (int c = 0; c < 3; ++c) r[3 * i + c] = fd[c];
        ri[2 + i] = a.qstatus[(size_t)sc * n + i];
        if (i == 0) {
          double ref[6];  // x_ref, v_ref of the law in force at the HL instant
          if (a.track) {
            double ar[3];
            track_references(track_of(a, sc), track_time(a.tick, a.dt), ref, ref + 3, ar);
          } else {
            double m[DAT_MOUNTAIN_SIZE];
            mountain_of(a, sc, m);
            forest_references(xl, m, REF_X_OFFSET, ref, ref + 3);
          }
          r[DAT_LOG_HL_MIND(n)] = a.mind[sc];
          for (int c = 0; c < 6; ++c) r[DAT_LOG_HL_XREF(n) + c] = lref[6 * ls + c] = ref[c];
          ri[0] = a.iters[sc];
          ri[1] = a.col[sc];
        }
      }
    }
    lslot[lane] = slot;
  }
  const double* J = prm + DAT_P_J(n) + 9 * i;
  const double* Ji = prm + DAT_P_JINV(n) + 9 * i;
  double* mine = xs + lane * RO_X;
  const double* grp = xs + ls * n * RO_X;
  for (int s = 0; s < steps; ++s) {
    double dw[3] = {0, 0, 0};
    if (valid) {
      double f, M[3];
      ll_control_agent(R, W, J, fd, &f, M, a.ll_kind);
      if constexpr (LOG) {
        if (s == lnext && lslot[lane] >= 0) {  // 32-byte aligned: two 16-byte stores
          double2* w = reinterpret_cast<double2*>(lrec + (size_t)lslot[lane] * DAT_LOG_ST_WORDS(n) + 4 * i);
          w[0] = make_double2(f, M[0]);
          w[1] = make_double2(M[1], M[2]);
        }
      }
      double um[RO_X];
      quad_accel(R, W, J, Ji, prm + DAT_P_RCOM(n) + 3 * i, Rl, f, M, dw, um);
      for (int c = 0; c < RO_X; ++c) mine[c] = um[c];
    }
    __syncthreads();
    if (valid) {
      double dvc[3] = {0, 0, 0}, mom[3] = {0, 0, 0}, dvl[3], dwl[3];
      for (int k = 0; k < n; ++k)
        for (int c = 0; c < 3; ++c) { dvc[c] += grp[k * RO_X + c]; mom[c] += grp[k * RO_X + 3 + c]; }
      payload_accel(prm, Rl, wl, dvc, mom, dvl, dwl);
      integrate_rot(R, W, dw, dt);
      integrate_lin(xl, vl, dvl, dt);
      integrate_rot(Rl, wl, dwl, dt);
      if (projection_due(&cnt)) {
        polar3(Rl);
        polar3(R);
      }
      if constexpr (LOG) {
        if (s == lnext && lslot[lane] >= 0) {
          double* rec = lrec + (size_t)lslot[lane] * DAT_LOG_ST_WORDS(n);
          double* q = rec + DAT_LOG_ST_STATE(n);
          for (int k = 0; k < 9; ++k) q[DAT_S_R(n) + 9 * i + k] = R[k];
          for (int c = 0; c < 3; ++c) q[DAT_S_W(n) + 3 * i + c] = W[c];
          if (i == 0) {
            const double* ref = lref + 6 * ls;
            double ex[3], ev[3];
            for (int c = 0; c < 3; ++c) {
              q[DAT_S_XL(n) + c] = xl[c];
              q[DAT_S_VL(n) + c] = vl[c];
              q[DAT_S_WL(n) + c] = wl[c];
              ex[c] = ref[c] - xl[c];
              ev[c] = ref[3 + c] - vl[c];
            }
            for (int k = 0; k < 9; ++k) q[DAT_S_RL(n) + k] = Rl[k];
            rec[DAT_LOG_ST_XERR(n)] = sqrt(dot3(ex, ex));
            rec[DAT_LOG_ST_XERR(n) + 1] = sqrt(dot3(ev, ev));
          }
        }
      }
    }
    if constexpr (LOG) {
      if (s == lnext) {
        lnext += lg.log_every;
        lrec += (size_t)lg.nslot * DAT_LOG_ST_WORDS(n);
      }
    }
    __syncthreads();  // the sums are read before the next step overwrites them
  }
  if (valid) {
    for (int k = 0; k < 9; ++k) g[DAT_S_R(n) + 9 * i + k] = R[k];
    for (int c = 0; c < 3; ++c) g[DAT_S_W(n) + 3 * i + c] = W[c];
    if (i == 0) {
      for (int c = 0; c < 3; ++c) {
        g[DAT_S_XL(n) + c] = xl[c];
        g[DAT_S_VL(n) + c] = vl[c];
        g[DAT_S_WL(n) + c] = wl[c];
      }
      for (int k = 0; k < 9; ++k) g[DAT_S_RL(n) + k] = Rl[k];
      a.counter[sc] = cnt;
      if constexpr (ADV == ADV_EARLY) a.adv[sc] = a.serial;
    }
  }
  return true;
}
template <bool LOG, int ADV, bool EP = false>
__global__ __launch_bounds__(64) void k_rollout_agents(KArgs a, int steps, double dt, const double* fdes,
                                                       std::conditional_t<LOG, LogArgs, NoLog> lg,
                                                       std::conditional_t<EP, EpArgs, NoEp> ep) {
  __shared__ double xs[64 * RO_X];
  bool took;
  (void)rollout_lanes<LOG, ADV, EP>(a, steps, dt, fdes, lg, xs, &took, ep);
}

// RQPLowLevelController.control (control/rqp_centralized.py:518-535) at the current states: thrust
// f (B x n) and moments M (B x n x 3) from f_des, one lane per (scenario, agent)
__global__ void k_low_level(KArgs a, const double* fdes, double* fo, double* Mo) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = a.n;
  if (t >= a.B * n) return;
  const int sc = t / n, i = t - sc * n;
  const double* prm = prm_of(a, sc);
  const double* st = a.state + (size_t)sc * a.S;
  // (inlined here as in the rollout instantiations: with three callers the inliner would leave a call)
  [[clang::always_inline]] ll_control_agent(st + DAT_S_R(n) + 9 * i, st + DAT_S_W(n) + 3 * i, prm + DAT_P_J(n) + 9 * i,
                                            fdes + (size_t)sc * 3 * n + 3 * i, fo + t, Mo + 3 * (size_t)t, a.ll_kind);
}

// rigid payload (system/rigid_payload.py:93-130): `steps` steps of dt with the forces f held, one lane per scenario
__global__ void k_rp_rollout(KArgs a, int steps, double dt, const double* f) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= a.B) return;
  const int n = a.n;
  const double* prm = prm_of(a, sc);
  double* st = a.state + (size_t)sc * a.S;
  int cnt = a.counter[sc];
  for (int s = 0; s < steps; ++s) rp_step(prm, n, st, &cnt, f + (size_t)sc * 3 * n, dt);
  a.counter[sc] = cnt;
}

__device__ __forceinline__ void desired_of(const KArgs& a, int sc, double* acc);  // (below, with k_desired)
// The rigid payload's advance pass of the resident closed loop (dat_set_plant DAT_PLANT_RP): the `steps` payload steps
// of an HL period under the forces k_cent has just published, k_rp_rollout's mapping (one lane per scenario), with the
// payload's state in registers, then the next step's desired acceleration (desired_of's two laws, at the launch's
// tick: the next step's) from those registers.  rp_step's pieces, in its order, so a step is rp_step's to the bit.
__global__ __launch_bounds__(64) void k_rp_advance(KArgs a, int steps, double dt, const double* f, double* acc) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= a.B) return;
  const int n = a.n;
  const double* prm = prm_of(a, sc);
  double* g = a.state + (size_t)sc * a.S;
  const double* fs = f + (size_t)sc * 3 * n;
  double xl[3], vl[3], Rl[9], wl[3];
  for (int c = 0; c < 3; ++c) {
    xl[c] = g[DAT_S_XL(n) + c];
    vl[c] = g[DAT_S_VL(n) + c];
    wl[c] = g[DAT_S_WL(n) + c];
  }
  for (int k = 0; k < 9; ++k) Rl[k] = g[DAT_S_RL(n) + k];
  int cnt = a.counter[sc];
  const double ml = prm[DAT_P_MT];
  const double* r = prm + DAT_P_RCOM(n);
  // the force sum does not change while the forces are held
  double F[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) F[c] += fs[3 * i + c];
  const double dvl[3] = {F[0] / ml, F[1] / ml, F[2] / ml - DAT_GRAVITY};
  for (int s = 0; s < steps; ++s) {
    double Mo[3] = {0, 0, 0}, dwl[3];
    for (int i = 0; i < n; ++i) {
      double fi[3] = {fs[3 * i], fs[3 * i + 1], fs[3 * i + 2]}, fb[3], m3[3];
      mtv3(Rl, fi, fb);
      cross3(r + 3 * i, fb, m3);
      for (int c = 0; c < 3; ++c) Mo[c] += m3[c];
    }
    rot_accel(prm + DAT_P_JT, prm + DAT_P_JTI, wl, Mo, dwl);
    integrate_lin(xl, vl, dvl, dt);
    integrate_rot(Rl, wl, dwl, dt);
    if (projection_due(&cnt)) polar3(Rl);
  }
  for (int c = 0; c < 3; ++c) {
    g[DAT_S_XL(n) + c] = xl[c];
    g[DAT_S_VL(n) + c] = vl[c];
    g[DAT_S_WL(n) + c] = wl[c];
  }
  for (int k = 0; k < 9; ++k) g[DAT_S_RL(n) + k] = Rl[k];
  a.counter[sc] = cnt;
  if (acc == nullptr) return;  // (the call's last step: the next call computes its own inputs)
  double* o = acc + (size_t)sc * 6;
  if (a.track) {
    desired_accel_track_at(xl, vl, track_of(a, sc), track_time(a.tick, a.dt), o);
  } else {
    desired_of(a, sc, acc);  // the forest law reads a state block: the one this lane has just stored
  }
}

// Point-mass rigid-link system (PMRLDynamics, system/point_mass_rigid_link.py:135-254; the pieces of
// dat_pmrl_step.hpp), k_rollout_agents' mapping: one lane per link, G = floor(64/n) scenarios per 64-lane block, idle
// lanes masked.  A lane holds its link (q, dq) and a copy of the payload in registers across the steps.  Per step one
// LDS exchange between one pair of barriers: lane i publishes (m_i, y_i, g_i); every lane of the scenario assembles
// S and G y from the records in link order (identical bits in all of them), solves the 6 x 6 system and integrates
// its own link and its copy of the payload.  Lane 0 of a scenario writes the payload and the counter back.
constexpr int PM_X = 8;  // per lane in LDS: m, y, g (6)
// the accelerations at the lane's state: the lane's T and ddq, the scenario's dvl and dwl (all lanes of a block
// call it, valid or not: it holds the step's two barriers)
__device__ __forceinline__ void pmrl_lane_forward(const double* prm, int n, int i, bool valid, double* mine,
                                                  const double* grp, const double* Rl, const double* wl,
                                                  const double* q, const double* dq, const double* f, double* T,
                                                  double* ddq, double* dvl, double* dwl) {
  PmrlPayload p;
  PmrlLink lk;
  if (valid) {
    pmrl_payload_terms(prm, Rl, wl, p);
    pmrl_link_terms(prm, n, i, p, Rl, q, dq, f, lk);
    mine[0] = prm[DAT_P_PM_M(n) + i];
    mine[1] = lk.y;
    for (int c = 0; c < 6; ++c) mine[2 + c] = lk.g[c];
  }
  __syncthreads();
  if (valid) {
    double S[21], z[6];
    pmrl_system_clear(S, z);
    for (int k = 0; k < n; ++k) {
      double rec[PM_X];
      for (int c = 0; c < PM_X; ++c) rec[c] = grp[k * PM_X + c];
      pmrl_system_add(S, z, rec[0], rec[1], rec + 2);
    }
    pmrl_solve6(S, z);
    PmrlSums s;
    pmrl_payload_accel(prm, n, p, z, s, dvl, dwl);
    *T = pmrl_tension(prm[DAT_P_PM_M(n) + i], lk.y, lk.g, z);
    pmrl_link_accel(prm, n, i, Rl, lk, q, *T, s, ddq);
  }
  __syncthreads();  // the records are read before the next step overwrites them
}
// `steps` steps of dt under the force schedule f[nf][B][3n] (agent-major): step s uses set s / (steps / nf)
__global__ __launch_bounds__(64) void k_pmrl_rollout(KArgs a, int steps, int nf, double dt, const double* f) {
  __shared__ double xs[64 * PM_X];
  const int n = a.n, G = 64 / n, NT = G * n;
  const int lane = threadIdx.x, ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  const bool valid = lane < NT && sc < a.B;
  const double* prm = valid ? prm_of(a, sc) : a.params;
  double* g = valid ? a.state + (size_t)sc * a.S : nullptr;
  double q[3] = {0, 0, 1}, dq[3] = {0, 0, 0}, xl[3], vl[3], Rl[9], wl[3], fi[3] = {0, 0, 0};
  int cnt = 0;
  if (valid) {
    for (int c = 0; c < 3; ++c) {
      q[c] = g[DAT_S_Q(n) + 3 * i + c];
      dq[c] = g[DAT_S_DQ(n) + 3 * i + c];
      xl[c] = g[DAT_S_XL(n) + c];
      vl[c] = g[DAT_S_VL(n) + c];
      wl[c] = g[DAT_S_WL(n) + c];
    }
    for (int k = 0; k < 9; ++k) Rl[k] = g[DAT_S_RL(n) + k];
    cnt = a.counter[sc];
  }
  const int hold = steps / nf;  // steps a force set is held
  const size_t fset = (size_t)a.B * 3 * n;
  const double* fp = f + (valid ? (size_t)sc * 3 * n + 3 * i : 0);
  for (int s = 0, left = 0; s < steps; ++s, --left) {
    if (left == 0) {
      left = hold;
      if (valid)
        for (int c = 0; c < 3; ++c) fi[c] = fp[c];
      fp += fset;
    }
    double T, ddq[3], dvl[3], dwl[3];
    pmrl_lane_forward(prm, n, i, valid, xs + lane * PM_X, xs + ls * n * PM_X, Rl, wl, q, dq, fi, &T, ddq, dvl, dwl);
    if (valid) {
      pmrl_integrate_link(q, dq, ddq, dt);
      pmrl_integrate_payload(xl, vl, Rl, wl, dvl, dwl, dt, &cnt);
    }
  }
  if (valid) {
    for (int c = 0; c < 3; ++c) {
      g[DAT_S_Q(n) + 3 * i + c] = q[c];
      g[DAT_S_DQ(n) + 3 * i + c] = dq[c];
    }
    if (i == 0) {
      for (int c = 0; c < 3; ++c) {
        g[DAT_S_XL(n) + c] = xl[c];
        g[DAT_S_VL(n) + c] = vl[c];
        g[DAT_S_WL(n) + c] = wl[c];
      }
      for (int k = 0; k < 9; ++k) g[DAT_S_RL(n) + k] = Rl[k];
      a.counter[sc] = cnt;
    }
  }
}
// PMRLDynamics.forward_dynamics (:156-208) at the current states, which it leaves alone: ddq (B x 3n, agent-major),
// dvl, dwl (B x 3), T (B x n) under the thrusts f (B x 3n)
__global__ __launch_bounds__(64) void k_pmrl_forward(KArgs a, const double* f, double* ddq_o, double* dvl_o,
                                                     double* dwl_o, double* T_o) {
  __shared__ double xs[64 * PM_X];
  const int n = a.n, G = 64 / n, NT = G * n;
  const int lane = threadIdx.x, ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  const bool valid = lane < NT && sc < a.B;
  const double* prm = valid ? prm_of(a, sc) : a.params;
  const double* g = valid ? a.state + (size_t)sc * a.S : nullptr;
  double q[3] = {0, 0, 1}, dq[3] = {0, 0, 0}, Rl[9], wl[3], fi[3] = {0, 0, 0};
  if (valid) {
    for (int c = 0; c < 3; ++c) {
      q[c] = g[DAT_S_Q(n) + 3 * i + c];
      dq[c] = g[DAT_S_DQ(n) + 3 * i + c];
      wl[c] = g[DAT_S_WL(n) + c];
      fi[c] = f[(size_t)sc * 3 * n + 3 * i + c];
    }
    for (int k = 0; k < 9; ++k) Rl[k] = g[DAT_S_RL(n) + k];
  }
  double T, ddq[3], dvl[3], dwl[3];
  pmrl_lane_forward(prm, n, i, valid, xs + lane * PM_X, xs + ls * n * PM_X, Rl, wl, q, dq, fi, &T, ddq, dvl, dwl);
  if (valid) {
    for (int c = 0; c < 3; ++c) ddq_o[(size_t)sc * 3 * n + 3 * i + c] = ddq[c];
    T_o[(size_t)sc * n + i] = T;
    if (i == 0)
      for (int c = 0; c < 3; ++c) {
        dvl_o[(size_t)sc * 3 + c] = dvl[c];
        dwl_o[(size_t)sc * 3 + c] = dwl[c];
      }
  }
}

// the desired acceleration of scenario sc from its state in memory (k_desired, k_advance): the tracking law at the
// launch's tick where records are set (uniform per launch), else the forest law
__device__ __forceinline__ void desired_of(const KArgs& a, int sc, double* acc) {
  const double* st = a.state + (size_t)sc * a.S;
  double* o = acc + (size_t)sc * 6;
  if (a.track) {
    desired_accel_track(st, a.n, track_of(a, sc), track_time(a.tick, a.dt), o);
    return;
  }
  double m[DAT_MOUNTAIN_SIZE];
  mountain_of(a, sc, m);
  desired_accel_forest(st, a.n, m, REF_X_OFFSET, o);
}
template <int ADV>
__global__ void k_desired(KArgs a, double* acc) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= a.B || !adv_gate<ADV, false>(a, sc)) return;
  desired_of(a, sc, acc);
}

// The advance pass of the closed loop in one launch (dat_set_fused_advance): k_rollout_agents<false, ADV>, k_desired<ADV>
// and k_env_class<ADV> of a block's G scenarios, through the same device functions on the same inputs, so a
// scenario's state, acc, env rows and key are bit for bit those of the three launches.  The three share the mapping
// (lane ls * n + i: agent i) and the gate: the scenarios the rollout takes are the ones it marks (ADV_EARLY) or
// finds unmarked (ADV_REST), which is the gate of the other two.  The block barrier orders the state's write-back
// before its reads: k_desired's by the scenario's first lane, the env rows' by every lane, from memory as in the
// separate kernels.  One grid waits once for the SIMDs the drain's wavefronts free, and the state is not fetched
// from memory again.  Registers: bound as k_env_class (256); the rollout's are dead at the barrier.
// EP: with episodes open (rollout_lanes): a scenario respawned instead of rolled out gets its next inputs from the new state.
template <int ADV, bool EP = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_advance(
    KArgs a, int steps, double dt, const double* fdes, double* acc, int* kc_lo, int* kc_hi,
    std::conditional_t<EP, EpArgs, NoEp> ep) {
  static_assert(ADV == ADV_EARLY || ADV == ADV_REST, "the ungated step runs the three kernels");
  __shared__ double xs[64 * RO_X];
  __shared__ int nd[64], cl[64];
  __shared__ double md[64];
  __shared__ double ent[64 * ENV_CS];
  const int n = a.n, G = 64 / n;
  const int lane = threadIdx.x, ls = lane / n, i = lane - ls * n;
  const int sc = blockIdx.x * G + ls;
  bool valid;
  if (!rollout_lanes<false, ADV, EP>(a, steps, dt, fdes, NoLog{}, xs, &valid, ep)) return;
  __syncthreads();  // the state is stored before it is read back
  if (valid && i == 0) desired_of(a, sc, acc);
  double lhs[DAT_NENV][3], rhs[DAT_NENV];
  env_class_lanes<ADV>(a, n, lane, ls, i, sc, valid, nd, cl, md, ent, lhs, rhs);
  // the sort's count (k_bucket_scatter), where the keys are made: the block's histogram, then one atomic per key it
  // holds into the key table of the list the scenario goes to (kc_lo: keys below NKEY, kc_hi: the tail-routed ones;
  // null: the sort counts for itself)
  if (kc_lo == nullptr) return;
  __shared__ int hist[NKEY_ALL];
  for (int k = lane; k < NKEY_ALL; k += 64) hist[k] = 0;
  __syncthreads();
  if (valid && i == 0) atomicAdd(&hist[sort_key(a.need[sc])], 1);  // (the key this lane has just stored)
  __syncthreads();
  for (int k = lane; k < NKEY_ALL; k += 64)
    if (const int c = hist[k]) atomicAdd((k < NKEY ? kc_lo : kc_hi) + KT_COUNT + k, c);
}

__global__ void k_warm(KArgs a) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc >= a.B) return;
  const int n = a.n, N3 = 3 * n;
  const double* prm = prm_of(a, sc);
  const double* feq = prm + DAT_P_FEQ(n);
  if (a.cf) {
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < N3; ++c) {
        a.cf[((size_t)sc * n + i) * N3 + c] = feq[c];
        a.clam[((size_t)sc * n + i) * N3 + c] = 0.0;
      }
    for (int c = 0; c < N3; ++c) a.cfbar[(size_t)sc * N3 + c] = feq[c];
  }
  if (a.dlamF) {
    double s3[3] = {0, 0, 0};
    for (int k = 0; k < n; ++k)
      for (int c = 0; c < 3; ++c) s3[c] += feq[3 * k + c];
    for (int c = 0; c < N3; ++c) { a.dlamF[(size_t)sc * N3 + c] = 0.0; a.dlamM[(size_t)sc * N3 + c] = 0.0; }
    for (int i = 0; i < n; ++i) dd_fallback(prm, n, i, s3, a.dprev + ((size_t)sc * n + i) * 9);
  }
  if (a.pf)
    for (int c = 0; c < N3; ++c) a.pf[(size_t)sc * N3 + c] = feq[c];
  for (int c = 0; c < N3; ++c) a.fdes[(size_t)sc * N3 + c] = feq[c];
  // the previous step's ADMM / DD iteration count and slowest IPM count select the IPM start (C-ADMM
  // warm regime) and the drain order: a reset handle behaves exactly like a freshly created one
  a.iters[sc] = 0;
  if (a.ipmx) a.ipmx[sc] = 0;
}

__global__ void k_env(KArgs a, double* lhs, double* rhs, int* nrow, unsigned char* col, double* md) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = a.n;
  if (t >= a.B * n) return;
  const int sc = t / n, i = t % n;
  const double* prm = prm_of(a, sc);
  const double* st = a.state + (size_t)sc * a.S;
  const double* trees;
  int nt, k = 0;
  unsigned mask;
  forest_of(a, sc, &trees, &nt);
  double L[DAT_NENV][3], R[DAT_NENV];
  bool cent = (a.cf == nullptr && a.dlamF == nullptr);
  EnvOut e = env_rows(prm, n, st, trees, nt, cent ? -1 : i, cent ? prm[DAT_P_AENVC] : prm[DAT_P_AENVD], &mask, L, R);
  double* lo = lhs + (size_t)t * DAT_NENV * 3;
  double* ro = rhs + (size_t)t * DAT_NENV;
  for (int r = 0; r < DAT_NENV; ++r) {
    for (int c = 0; c < 3; ++c) lo[3 * r + c] = 0.0;
    ro[r] = 0.0;
  }
#pragma unroll
  for (int r = 0; r < DAT_NENV; ++r) {
    if (!((mask >> r) & 1u)) continue;
    for (int c = 0; c < 3; ++c) lo[3 * k + c] = L[r][c];
    ro[k] = R[r];
    ++k;
  }
  nrow[t] = k;
  col[t] = (unsigned char)e.collision;
  md[t] = e.min_env_dist;
}

// ------------------------------------------------------------------------------------------------
// checkpoint records (dat_checkpoint_save / dat_checkpoint_load; layout: dat_layout.h DAT_CK_*)
// ------------------------------------------------------------------------------------------------
// the kernels' argument type, named as it was when the kernels got their symbols: dat::CkArgs's fields
struct CkArgs : dat::CkArgs {
  CkArgs(const dat::CkArgs& c) : dat::CkArgs(c) {}
};
template <int U>
struct CkUnit;
template <>
struct CkUnit<1> { using T = double; };
template <>
struct CkUnit<2> { using T = double2; };
// the array and the word in it behind word x of scenario sc's record (null: an int word or padding)
__device__ __forceinline__ double* ck_word(const CkArgs& c, int sc, int x) {
  for (int k = 0; k < c.nf; ++k) {
    const int d = x - c.off[k];
    if ((unsigned)d < (unsigned)c.w[k]) return c.f[k] + (size_t)sc * c.w[k] + d;
  }
  return nullptr;
}
// One wavefront per record; its lanes walk the record's words in units of U words (U = 2, 16-byte accesses, where
// every segment's size and offset is even: every source run and every record is then 16-byte aligned; else U = 1),
// so a wavefront instruction reads and writes runs of up to 1 KiB / 512 B that are contiguous within a segment.
// k_ckpt_gather: record r of `out` from scenario list[r] (null: r).
template <int U>
__global__ __launch_bounds__(256) void k_ckpt_gather(CkArgs c, const int* list, int count, double* out) {
  using T = typename CkUnit<U>::T;
  const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
  const long long r = (long long)blockIdx.x * wpb + (threadIdx.x >> 6);
  if (r < count) {
    const int sc = list ? list[r] : (int)r;
    double* rec = out + (size_t)r * c.words;
    for (int x = lane * U; x < c.words; x += 64 * U) {
      double v[2] = {0.0, 0.0};
      if ((unsigned)(x - c.ints_off) < (unsigned)CK_INT_WORDS) {
        for (int j = 0; j < U; ++j) {
          const int i0 = 2 * (x + j - c.ints_off);
          v[j] = __hiloint2double(c.ints[i0 + 1] ? c.ints[i0 + 1][sc] : 0, c.ints[i0] ? c.ints[i0][sc] : 0);
        }
      } else if (const double* p = ck_word(c, sc, x)) {
        const T t = *(const T*)p;
        memcpy(v, &t, sizeof(T));
      }
      T t;
      memcpy(&t, v, sizeof(T));
      *(T*)(rec + x) = t;
    }
  }
}
// k_ckpt_scatter: record rec[r] - base (null: r - base) of `in` into scenario scen[r] (null: r); the scenarios are
// distinct.  Their stamps are cleared: 0 is no step's stamp (next_serial).
template <int U>
__global__ __launch_bounds__(256) void k_ckpt_scatter(CkArgs c, const double* in, const int* recs, const int* scen,
                                                      int base, int count) {
  using T = typename CkUnit<U>::T;
  const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
  const long long r = (long long)blockIdx.x * wpb + (threadIdx.x >> 6);
  if (r < count) {
    const int sc = scen ? scen[r] : (int)r;
    const double* rec = in + (size_t)((recs ? recs[r] : (int)r) - base) * c.words;
    for (int x = lane * U; x < c.words; x += 64 * U) {
      const T t = *(const T*)(rec + x);
      double v[2] = {0.0, 0.0};
      memcpy(v, &t, sizeof(T));
      if ((unsigned)(x - c.ints_off) < (unsigned)CK_INT_WORDS) {
        for (int j = 0; j < U; ++j) {
          const int i0 = 2 * (x + j - c.ints_off);
          if (c.ints[i0]) c.ints[i0][sc] = __double2loint(v[j]);
          if (c.ints[i0 + 1]) c.ints[i0 + 1][sc] = __double2hiint(v[j]);
        }
      } else if (double* p = ck_word(c, sc, x)) {
        *(T*)p = t;
      }
    }
    if (lane == 0 && c.done) c.done[sc] = 0;
    if (lane == 0 && c.adv) c.adv[sc] = 0;
  }
}

}  // namespace

namespace dat {

static_assert(ADV_ALL == 0 && ADV_EARLY == 1 && ADV_REST == 2, "the launchers' tables are indexed by the mode");

hipError_t launch_k_desired(int adv, hipStream_t st, const KArgs& a, double* acc) {
  static constexpr void (*ks[])(KArgs, double*) = {k_desired<ADV_ALL>, k_desired<ADV_EARLY>, k_desired<ADV_REST>};
  hipLaunchKernelGGL(ks[adv], dim3((a.B + 63) / 64), dim3(64), 0, st, a, acc);
  return hipGetLastError();
}
hipError_t launch_k_env_class(int adv, int blocks, hipStream_t st, const KArgs& a) {
  static constexpr void (*ks[])(KArgs) = {k_env_class<ADV_ALL>, k_env_class<ADV_EARLY>, k_env_class<ADV_REST>};
  hipLaunchKernelGGL(ks[adv], dim3(blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_k_bucket(hipStream_t st, int B, const int* need, int* list, int* count) {
  hipLaunchKernelGGL(k_bucket, dim3(1), dim3(BUCKET_T), 0, st, B, need, list, count);
  return hipGetLastError();
}
hipError_t launch_k_bucket_adv(int adv, hipStream_t st, int B, const int* need, int* list, int* count, const int* advp,
                               int serial) {
  hipLaunchKernelGGL(adv == ADV_EARLY ? k_bucket_adv<ADV_EARLY> : k_bucket_adv<ADV_REST>, dim3(1), dim3(BUCKET_T), 0,
                     st, B, need, list, count, advp, serial);
  return hipGetLastError();
}
hipError_t launch_k_bucket_scatter(int adv, hipStream_t st, int B, const int* need, int* list, int* count,
                                   const int* advp, int serial, int* tab, int* other) {
  hipLaunchKernelGGL(adv == ADV_EARLY ? k_bucket_scatter<ADV_EARLY> : k_bucket_scatter<ADV_REST>,
                     dim3((B + SCATTER_T - 1) / SCATTER_T), dim3(SCATTER_T), 0, st, B, need, list, count, advp, serial,
                     tab, other);
  return hipGetLastError();
}
hipError_t launch_k_rollout_agents(const LogArgs* lg, int adv, int blocks, hipStream_t st, const KArgs& a, int steps,
                                   double dt, const double* fdes, const EpArgs* ep) {
  constexpr auto k_log = k_rollout_agents<true, ADV_ALL>;
  constexpr auto k_all = k_rollout_agents<false, ADV_ALL>;
  constexpr auto k_early = k_rollout_agents<false, ADV_EARLY>;
  constexpr auto k_rest = k_rollout_agents<false, ADV_REST>;
  constexpr auto e_all = k_rollout_agents<false, ADV_ALL, true>;
  constexpr auto e_early = k_rollout_agents<false, ADV_EARLY, true>;
  constexpr auto e_rest = k_rollout_agents<false, ADV_REST, true>;
  if (lg && ep) return hipErrorInvalidValue;  // (dat_episode_begin and dat_log_begin exclude each other)
  if (lg)
    hipLaunchKernelGGL(k_log, dim3(blocks), dim3(64), 0, st, a, steps, dt, fdes, *lg, NoEp{});
  else if (ep)
    hipLaunchKernelGGL(adv == ADV_EARLY ? e_early : adv == ADV_REST ? e_rest : e_all, dim3(blocks), dim3(64), 0, st, a,
                       steps, dt, fdes, NoLog{}, *ep);
  else
    hipLaunchKernelGGL(adv == ADV_EARLY ? k_early : adv == ADV_REST ? k_rest : k_all, dim3(blocks), dim3(64), 0, st, a,
                       steps, dt, fdes, NoLog{}, NoEp{});
  return hipGetLastError();
}
hipError_t launch_k_advance(int adv, int blocks, hipStream_t st, const KArgs& a, int steps, double dt,
                            const double* fdes, double* acc, int* kc_lo, int* kc_hi, const EpArgs* ep) {
  constexpr auto e_early = k_advance<ADV_EARLY, true>;
  constexpr auto e_rest = k_advance<ADV_REST, true>;
  if (ep)
    hipLaunchKernelGGL(adv == ADV_EARLY ? e_early : e_rest, dim3(blocks), dim3(64), 0, st, a, steps, dt, fdes, acc,
                       kc_lo, kc_hi, *ep);
  else
    hipLaunchKernelGGL(adv == ADV_EARLY ? k_advance<ADV_EARLY> : k_advance<ADV_REST>, dim3(blocks), dim3(64), 0, st, a,
                       steps, dt, fdes, acc, kc_lo, kc_hi, NoEp{});
  return hipGetLastError();
}
hipError_t launch_k_low_level(hipStream_t st, const KArgs& a, const double* fdes, double* fo, double* Mo) {
  hipLaunchKernelGGL(k_low_level, dim3((a.B * a.n + 63) / 64), dim3(64), 0, st, a, fdes, fo, Mo);
  return hipGetLastError();
}
hipError_t launch_k_rp_rollout(hipStream_t st, const KArgs& a, int steps, double dt, const double* f) {
  hipLaunchKernelGGL(k_rp_rollout, dim3((a.B + 63) / 64), dim3(64), 0, st, a, steps, dt, f);
  return hipGetLastError();
}
hipError_t launch_k_rp_advance(hipStream_t st, const KArgs& a, int steps, double dt, const double* f, double* acc) {
  hipLaunchKernelGGL(k_rp_advance, dim3((a.B + 63) / 64), dim3(64), 0, st, a, steps, dt, f, acc);
  return hipGetLastError();
}
hipError_t launch_k_pmrl_rollout(int blocks, hipStream_t st, const KArgs& a, int steps, int nf, double dt,
                                 const double* f) {
  hipLaunchKernelGGL(k_pmrl_rollout, dim3(blocks), dim3(64), 0, st, a, steps, nf, dt, f);
  return hipGetLastError();
}
hipError_t launch_k_pmrl_forward(int blocks, hipStream_t st, const KArgs& a, const double* f, double* ddq, double* dvl,
                                 double* dwl, double* T) {
  hipLaunchKernelGGL(k_pmrl_forward, dim3(blocks), dim3(64), 0, st, a, f, ddq, dvl, dwl, T);
  return hipGetLastError();
}
hipError_t launch_k_warm(hipStream_t st, const KArgs& a) {
  hipLaunchKernelGGL(k_warm, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_k_env(hipStream_t st, const KArgs& a, double* lhs, double* rhs, int* nrow, unsigned char* col,
                        double* md) {
  hipLaunchKernelGGL(k_env, dim3((a.B * a.n + 63) / 64), dim3(64), 0, st, a, lhs, rhs, nrow, col, md);
  return hipGetLastError();
}
// four wavefronts, one record each, per block
hipError_t launch_k_ckpt_gather(bool wide, hipStream_t st, const CkArgs& c, const int* list, int count, double* out) {
  hipLaunchKernelGGL(wide ? k_ckpt_gather<2> : k_ckpt_gather<1>, dim3((int)(((long long)count + 3) / 4)), dim3(256), 0,
                     st, c, list, count, out);
  return hipGetLastError();
}
hipError_t launch_k_ckpt_scatter(bool wide, hipStream_t st, const CkArgs& c, const double* in, const int* recs,
                                 const int* scen, int base, int count) {
  hipLaunchKernelGGL(wide ? k_ckpt_scatter<2> : k_ckpt_scatter<1>, dim3((int)(((long long)count + 3) / 4)), dim3(256),
                     0, st, c, in, recs, scen, base, count);
  return hipGetLastError();
}

}  // namespace dat
