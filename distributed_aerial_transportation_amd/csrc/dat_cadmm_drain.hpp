// dat_cadmm_drain.hpp -- the C-ADMM drain (cadmm_drain<CLS, RB, ADV, RMODE>), its LDS carve and the kernel templates
// k_cadmm<ADV, RMS> / k_cadmm0<ADV, RM0>.  Three units instantiate it, each a share of the device code that compiles beside the
// others: dat_k_cadmm.hip (ADV = false), dat_k_cadmm_adv.hip (ADV = true) and dat_k_cadmm_tail.hip (RB = true).
#pragma once

#include "dat_cadmm_lds.hpp"

#ifdef DAT_CAPTURE_LOOSE
// development builds only (tools/capture_loose.py): the inputs of the tail's agent QPs accepted in band beyond
// Clarabel's 1e-8 -- [0] scenario, [1] agent, [2] ADMM pass, [3] rho, [4] previous step's passes, [5] forest,
// [6] merit, [7] fused step, [8, 14) acc_des, then the state (S), the agent's multipliers (3n) and the mean (3n)
namespace dat {
constexpr int CAP_MAX = 64, CAP_DOUBLES = 320;
__device__ double g_cap[CAP_MAX][CAP_DOUBLES];
__device__ unsigned int g_ncap;
}  // namespace dat
#endif

// Internal linkage, as in the one unit this text came from: each unit's inliner weighs these functions as it did
// there, and a kernel keeps its symbol.
namespace {
using namespace dat;

struct CadmmLds {
  double *fbar, *Rt, *red, *rows;
  QPShared* sh;
  double* env;
  int* done;  // per slot: the scenario stopped in this pass
  int* sid;   // per slot: scenario id, -1 empty, -2 retired (queue drained)
  int* wmx;   // per slot: IPM iterations of the scenario's slowest agent QP so far this step
};
__device__ inline CadmmLds cadmm_carve(double* smem, int n, int G, int cls, int rmode) {
  CadmmLds L;
  L.fbar = smem;
  L.Rt = L.fbar + al2(G * 3 * n);
  L.sh = (QPShared*)(L.Rt + G * RT_STRIDE * n);
  L.done = (int*)(L.sh + G);
  L.sid = L.done + G;
  L.wmx = L.sid + G;
  L.rows = (double*)(L.done + slot_ints(G));
  L.red = L.rows;
  const int ra = rmode ? row_lds_doubles(cadmm_nr(cls), cadmm_aux_doubles(cls, rmode)) : 0;
  L.env = L.rows + (ra > 64 * RDS ? ra : 64 * RDS);
  return L;
}

// A persistent 64-lane block drains the queue of env class CLS (the class's stretch of the sorted
// scenario list, claimed one scenario at a time through the class's queue head).  The block holds G scenario
// slots of n lanes; a slot whose scenario stops is refilled with the next scenario of the queue at
// the start of the next ADMM pass, so a wavefront no longer idles until its slowest scenario of a
// fixed group stops (SIMD occupancy: dat_get_class_occupancy).  A scenario's arithmetic does not
// depend on which slot or wavefront runs it.
// Every agent QP is solved as ipm_solve IPM_FAST_REDO defines it: the fast solver, redone by the robust one
// when it does not end cleanly (ipm_unclean).  RB = false (k_cadmm) carries only the fast solver (IPM_FAST): a
// scenario one of whose agent QPs does not end cleanly leaves at the end of that pass's solves with a resume
// record (rres) and goes to its class's hand-over list; so does a scenario whose next pass falls under the tail
// rule (tail_rule, dat_cadmm_step.hpp), at the end of the pass before it.  RB = true (k_cadmm_tail: one
// scenario slot per wavefront) drains the hand-over lists after k_cadmm (tmode 0), resuming each scenario in
// the pass it left (re-solving there only the agent QPs handed over), or the scenarios k_env_class routed to the
// tail before the step, concurrently with k_cadmm (tmode 1), and finishes their steps (and later fused steps).
// The tail's solves: IPM_FAST_REDO with the certificate of infeasible rows (dvl_rows_infeasible, once per
// scenario-step) and, in the passes the tail rule names, the warm start from the agent QP's converged iterate of
// the previous pass and the stall exit (ipm_solve WS).  Built with -ffp-contract=on (multiply-adds fused within
// an expression only), the inlined fast solver computes the same bits in either kernel, and the tail rule
// depends on the scenario's own history: a scenario's results do not depend on which kernel ran which pass.
// ADV: the drain of the closed loop's advance overlap (dat_closed_loop): a stopped scenario's f_des, iters and
// ipmx are stored write-through and stamped in KArgs::done, and k_cadmm's class-0 drain tells the host when its
// queue has been claimed empty.  Without it k_cadmm / k_cadmm0 are compiled without any of that; the tail kernels
// exist once and go by KArgs::done at run time (a second instantiation changes how their solver is inlined).
// RMODE: the row placement of the class's IPM (dat_cadmm_lds.hpp: 0 registers, 1 LDS rows, 2 LDS rows + the class's
// aux slots; the tail: 3), fixed at compile time -- the drain carries the one ipm_solve instantiation it runs, and
// the host launches the kernel of the word it sized the carve by (cadmm_row_modes, launch_cadmm).
template <int CLS, bool RB, bool ADV, int RMODE>
__device__ __forceinline__ void cadmm_drain(const KArgs& a) {
  static_assert(RB ? RMODE == 3 : RMODE >= 0 && RMODE <= 2, "row mode");
  static_assert(RB || RMODE == 0 || CLS < NCLS - 1, "class 3 keeps its rows in registers");
  static_assert(RMODE != 2 || cadmm_auxm(CLS) != 0, "mode 2 needs aux slots");
  static_assert(RB || RMODE != 1 || CLS >= ROWLDS_MIN_CLS, "LDS rows without aux slots: classes ROWLDS_MIN_CLS up");
  constexpr bool ENV = CLS > 0;
  constexpr int NR = cadmm_nr(CLS);
  constexpr int NE = class_env_rows(CLS);
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int n = a.n, N3 = 3 * n;
  const int G = a.G;  // G <= 64 / n scenario slots (cadmm_slots); the tail: G = 1
  // the tail: V bit-identical clones of each agent lane (clone vi = lane / n) run the agent QP's solve in lockstep
  // and share out its stiff-row columns (ipm_attempt); only clone 0 writes the scenario's outputs
  const int V = RB ? tail_clones(n) : 1;
  const int NT = (RB ? V : G) * n;
  const int lane = threadIdx.x;
  const int vi = RB ? lane / n : 0;
  const int ls = RB ? 0 : lane / n, i = lane - (RB ? vi : ls) * n;
  const int al = RB ? i : lane;  // the lane's column in the row / env / aux images (a clone's: its agent's)
  const int lsc = ls < G ? ls : 0;
  const bool TM = RB && a.tmode == 1;  // the tail-routed stretch of slist (k_env_class), not the hand-over list
  const int first = a.scount[sc_at(TM ? SC_TAIL_START : SC_START, CLS)];
  const int cnt = a.scount[sc_at(TM ? SC_TAIL_SIZE : RB ? SC_HAND_SIZE : SC_SIZE, CLS)];
  if (cnt == 0) {
    // (an empty class 0 is claimed empty from the start: the advance overlap's signal, see the refill)
    if constexpr (ADV && !RB && CLS == 0)
      if (blockIdx.x == 0 && lane == 0)
        __hip_atomic_store(a.qempty, a.serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  int* const qh = a.scount + sc_at(TM ? SC_TAIL_HEAD : RB ? SC_HAND_HEAD : SC_HEAD, CLS);
  const int* const ql = (RB && !TM ? a.rlist : a.slist) + first;
  CadmmLds L = cadmm_carve(smem, n, G, CLS, RMODE);
  double* fb = L.fbar + lsc * N3;
  double* rts = L.Rt + lsc * RT_STRIDE * n;
  double* myred = L.red + lane * RDS;
  QPShared& S = L.sh[lsc];
  const LdsRef<QPShared> shr{L.sh, lsc};
  const EnvLdsN<NE> err{L.env, al};
  const RtLds rtr{L.Rt, (lsc * n + i) * RT_STRIDE};
  if (lane < G) L.sid[lane] = -1;
  __syncthreads();

  // per-lane state of the slot's current scenario
  DAT_PHASE_INIT(9);
  QPLane<1> P;
  int sc = -1;  // scenario of this lane's slot (-1: empty)
  const double* prm = nullptr;
  double* lam = nullptr;
  double* cfs = nullptr;  // the scenario's n agent copies f^(j), in the warm-state array (HBM / L2)
  double* myf = nullptr;
  double* bst = nullptr;
  double* wrl = nullptr;  // k_cadmm_tail: the lane's warm-start record
  int iter = 0, prev_iter = 0, qstat = ST_OPTIMAL;
  int kstep = 0;  // fused control steps (dat_control_steps): the slot scenario's current step
  int rmask = -1;  // k_cadmm_tail: the lanes that solve in the current pass (a resumed pass: those handed over)
  double rho = a.rho0;
  // the slot's QPShared is to be built at the top of the next pass: a new scenario, or a fused next step of the
  // same one.  One site, so build_shared_inl is inlined once and both compute the same bits.
  bool rebuild = false;
  WaveCounters wc;
  for (;;) {
    // ---- refill empty slots from the queue
    DAT_PHASE(11);
    if (lane < NT && i == 0 && vi == 0 && L.sid[ls] == -1) {
      const int q = atomicAdd(qh, 1);
      const int s2 = q < cnt ? ql[q] : -2;  // -2: queue drained, slot retires
      // the advance overlap: the first claim past the end of k_cadmm's last queue tells the host that most of the
      // batch is finished and the launch is ramping down (one system-scope store to mapped host memory)
      if constexpr (ADV && !RB && CLS == 0)
        if (q == cnt) __hip_atomic_store(a.qempty, a.serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      L.sid[ls] = s2;
      L.done[ls] = 0;
      L.wmx[ls] = RB && !TM && s2 >= 0 ? a.rres[(size_t)s2 * RRES_INTS + RRES_WMX] : 0;
    }
    __syncthreads();
    const int slot_sc = lane < NT ? L.sid[ls] : -2;
    const bool fresh = slot_sc >= 0 && slot_sc != sc;
    if (fresh) {
      sc = slot_sc;
      prm = prm_of(a, sc);
      const double* st = a.state + (size_t)sc * a.S;
      if (vi == 0) make_Rt(prm + DAT_P_RCOM(n) + 3 * i, st + DAT_S_RL(n), rts + RT_STRIDE * i);
      lam = a.clam + ((size_t)sc * n + i) * N3;
      cfs = a.cf + (size_t)sc * n * N3;
      myf = cfs + i * N3;
      if (vi == 0)
        for (int c = 0; c < 3; ++c) fb[3 * i + c] = a.cfbar[(size_t)sc * N3 + 3 * i + c];
      // (the tail: the lane's record in LDS, behind the env image -- a generic pointer, flat loads go to LDS)
      bst = RB ? L.env + env_lds_doubles(NE) + i * best_size(1) : a.best + ((size_t)sc * n + i) * BEST_REC;
      iter = 0;
      prev_iter = a.iters[sc];  // the previous step's ADMM iterations (rewritten when the scenario stops)
      qstat = ST_OPTIMAL;
      rho = a.rho0;
      kstep = 0;
      rmask = -1;
      if (RB) {
        wrl = a.wrec + ((size_t)sc * n + i) * WREC_SIZE;
        wrl[0] = 0.0;  // no recorded iterate yet
      }
      if (RB && !TM) {
        // where k_cadmm left the scenario (its warm state -- multipliers, copies, the mean -- is in place)
        const int* const rr = a.rres + (size_t)sc * RRES_INTS;
        kstep = rr[RRES_KSTEP];
        iter = rr[RRES_PASS];
        rmask = rr[RRES_LANES];
        for (int q = 0; q < iter; ++q) rho = cadmm_next_rho(rho, a.tau, a.rho_max);  // the pass's rho, as k_cadmm had it
        qstat = a.qstatus[(size_t)sc * n + i];  // the pass's status of a lane not solved again
      }
      rebuild = true;
    }
    if (rebuild) {
      rebuild = false;
      if (i == 0 && vi == 0)
        build_shared_inl(S, prm, n, a.state + (size_t)sc * a.S, a.acc + ((size_t)kstep * a.B + sc) * 6,
                         prm[DAT_P_KFD], prm[DAT_P_KMD], 3, true);
    }
    if (!__syncthreads_or(slot_sc >= 0)) break;  // every slot retired
    DAT_PHASE(12);
    if (fresh) {
      lane_cadmm_static(P, prm, i);
      if (ENV) {
        // the rows k_env_class computed from the same state this step
        const size_t NA = (size_t)a.B * n, g = (size_t)sc * n + i;
        const unsigned emask = a.emask[g];
        double lhs[DAT_NENV][3], rhs[DAT_NENV];
#pragma unroll
        for (int j = 0; j < DAT_NENV; ++j) {
          const bool on = (emask >> j) & 1u;  // unmarked slots are never written (set_env_rows skips them)
          lhs[j][0] = on ? a.erows[(4 * j + 0) * NA + g] : 0.0;
          lhs[j][1] = on ? a.erows[(4 * j + 1) * NA + g] : 0.0;
          lhs[j][2] = on ? a.erows[(4 * j + 2) * NA + g] : 0.0;
          rhs[j] = on ? a.erows[(4 * j + 3) * NA + g] : 0.0;
        }
        EnvRows E;
        set_env_rows(P, E, S, emask, lhs, rhs);
        env_to_lds<NE>(L.env, al, E);  // (clones: the same values to the same column)
        // the tail certifies infeasible rows once per scenario-step (such an agent QP would run 2 x 50 IPM
        // iterations in every pass and end INACCURATE: the previous solution is held either way)
        if (RB && cadmm_certify_rows(P, shr, err)) wc.cert += vi == 0;
      }
    }
    // ---- one ADMM pass of every occupied slot
    DAT_PHASE(14);
    bool active = slot_sc >= 0;
    int it_lane = 0;
    bool hand = false;  // k_cadmm: this lane's solve was not clean (ipm_unclean)
    // k_cadmm with sub-batches (no tail routing, KArgs::route): a wedged scenario leaves before its first pass, and
    // the tail runs its step from there, as it runs a routed one
    const bool wedged = !RB && iter == 0 && tail_wedged(prev_iter, a.tail_prev);
    if (active && wedged) hand = true;
    if (active && !wedged && ((rmask >> i) & 1)) {
      lane_cadmm_dynamic(P, prm, n, i, rts, lam, fb, rho, RT_STRIDE);
      DAT_PHASE(15);
      P.tuned = cadmm_tuned_start(iter, prev_iter);
      double y[1][3], w[6];
      IPMOut o;
      DAT_PHASE(10);
      constexpr unsigned AUXM = cadmm_auxm(CLS);
      constexpr int RM = RB ? IPM_FAST_REDO : IPM_FAST;
      using SHT = LdsRef<QPShared>;
      using ERT = EnvLdsN<NE>;
      if constexpr (RB) {
        // the tail rule: warm start and stall exit in pass iter (the record is kept in every pass)
        const bool wson = tail_rule(iter, prev_iter, a.tail_prev, a.tail_pass);
        wc.warm += vi == 0 && wson && wrl[0] == 1.0;
        o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowLds, TAIL_AUXM, NoGrp, RM, true>(
            shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol, RowLds{L.rows, al},
            NoGrp{}, wrl, wson, vi, V);
        wc.stall += vi == 0 && o.why == 7;
#ifdef DAT_CAPTURE_LOOSE
        if (vi == 0 && inband_loose(o)) {
          const unsigned k = atomicAdd(&g_ncap, 1u);
          if (k < (unsigned)CAP_MAX && 14 + a.S + 6 * n <= CAP_DOUBLES) {
            double* c = g_cap[k];
            c[0] = sc; c[1] = i; c[2] = iter; c[3] = rho; c[4] = prev_iter;
            c[5] = a.scen_forest ? a.scen_forest[sc] : -1; c[6] = o.merit; c[7] = kstep;
            for (int q = 0; q < 6; ++q) c[8 + q] = a.acc[((size_t)kstep * a.B + sc) * 6 + q];
            for (int q = 0; q < a.S; ++q) c[14 + q] = a.state[(size_t)sc * a.S + q];
            for (int q = 0; q < N3; ++q) { c[14 + a.S + q] = lam[q]; c[14 + a.S + N3 + q] = fb[q]; }
          }
        }
#endif
      } else if constexpr (RMODE == 2) {
        o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowLds, AUXM, NoGrp, RM>(
            shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol, RowLds{L.rows, lane});
      } else if constexpr (RMODE == 1) {
        o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowLds, 0, NoGrp, RM>(
            shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol, RowLds{L.rows, lane});
      } else {
        o = ipm_solve<MODE_CADMM, 1, NR, SHT, ERT, RtLds, RowRegs, 0, NoGrp, RM>(
            shr, err, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER, a.qp_tol);
      }
      hand = !RB && ipm_unclean(o);
      DAT_PHASE(9);
      // a solve k_cadmm hands over is counted once, by k_cadmm_tail (its IPM_FAST_REDO runs the fast attempt
      // again): its discarded outcome here is neither an agent-QP solve nor an in-band accept
      const int keep = hand || vi > 0 ? 0 : 1;  // (nor do its iterations enter the pass's slot counts; nor a clone's)
      wc.ipm += keep * o.iters;
      wc.inband += keep * o.inband;
#ifdef DAT_ITER_HIST
      atomicAdd(&g_iter_hist[o.iters < 63 ? o.iters : 63], 1ull);
#endif
      wc.loose += keep * inband_loose(o);
      wc.refs += keep * o.refs;
      wc.corrs += keep * o.corrs;
      it_lane = keep * o.iters;
      wc.rowit += (long long)(keep * o.iters) * (__builtin_popcount(S.bmask) + __builtin_popcount(P.emask));
      wc.qp += keep;
      qstat = o.status;
      if (vi == 0) cadmm_take_solve(o, myf, y[0], rts, RT_STRIDE, lam, fb, rho, n, i, prm + DAT_P_FEQ(n));
    }
    DAT_PHASE(13);
    wc.slot += wave_max(it_lane);  // (the tail's passes: counted apart, CNT_TAIL)
    ++wc.pass;
    if (active) atomicMax(&L.wmx[ls], it_lane);
    rmask = -1;
    // the slot's lanes whose solve k_cadmm hands over (a ballot: the block is one wavefront)
    const unsigned long long hb = __ballot(hand);
    const int hmask = lane < NT ? (int)((hb >> (ls * n)) & ((1ull << n) - 1ull)) : 0;
    // k_cadmm hands the slot's scenario to k_cadmm_tail, which resumes it in pass `iter` and solves there the
    // agent QPs of `lanes`: the mean and the lanes' statuses go with it (multipliers and copies are in place), the
    // resume record, the class's hand-over list, and the slot is freed
    auto hand_over = [&](int lanes) __attribute__((always_inline)) {
      for (int c = 0; c < 3; ++c) a.cfbar[(size_t)sc * N3 + 3 * i + c] = fb[3 * i + c];
      a.qstatus[(size_t)sc * n + i] = qstat;
      if (i == 0) {
        int* const rr = a.rres + (size_t)sc * RRES_INTS;
        rr[RRES_KSTEP] = kstep;
        rr[RRES_PASS] = iter;
        rr[RRES_WMX] = L.wmx[ls];
        rr[RRES_LANES] = lanes;
        a.rlist[first + atomicAdd(a.scount + sc_at(SC_HAND_SIZE, CLS), 1)] = sc;
        L.sid[ls] = -1;
      }
    };
    __syncthreads();
    if (!RB && active && hmask) {
      // an agent QP of the pass was not clean: the tail redoes the pass's unclean solves (the mean of the pass's
      // start, the statuses of the pass's other solves)
      hand_over(hmask);
      active = false;
    }
    if (active) {
      ++iter;
      rho = cadmm_next_rho(rho, a.tau, a.rho_max);
      cadmm_mean_block(cfs, n, i, myred);
    }
    __syncthreads();
    if (active && vi == 0) {
      for (int c = 0; c < 3; ++c) fb[3 * i + c] = myred[c];
    }
    __syncthreads();
    if (active) {
      if (a.use_total_res) {
        myred[6] = cadmm_total_res(myf, fb, n);
      } else {
        cadmm_aggregate_res(cfs, myf, rts, RT_STRIDE, n, i, myred);
      }
    }
    __syncthreads();
    if (active && i == 0 && vi == 0) {
      const double res = cadmm_pass_residual(L.red + (ls * n) * RDS, RDS, n, a.use_total_res);
      const bool stop = cadmm_stop(res, a.res_tol, iter, a.max_iter);
      if (!stop && a.record_err && a.err) a.err[(size_t)sc * (a.max_iter + 1) + iter - 1] = res;
      L.done[ls] = stop ? 1 : 0;
    }
    __syncthreads();
    if (active) {
      if (!L.done[ls]) {
        if (vi == 0) cadmm_dual_update(lam, myf, fb, rho, n);
        // the tail rule holds from the next pass on: all lanes solve there (the mean of this pass goes with it)
        if (!RB && tail_rule(iter, prev_iter, a.tail_prev, a.tail_pass)) hand_over(-1);
      } else {
        // the scenario stopped: write its outputs and free the slot
        if (RB && i == 0 && vi == 0) {  // a scenario-step the tail finished (and, routed before the step, apart)
          atomicAdd(a.counters + CNT_ROB, 1ull);
          if (TM && kstep == 0) atomicAdd(a.counters + CNT_TAIL + 2, 1ull);
        }
        // (ADV: what the early rollout and env rows of the scenario read while this kernel still runs -- f_des,
        // iters, ipmx -- goes out write-through; the closed loop does not fuse steps, so this is the scenario's
        // last one)
        const bool wt = RB ? a.done != nullptr : ADV;  // (k_cadmm: fixed at compile time; the tail: per launch)
        if (vi == 0) {
          for (int c = 0; c < 3; ++c) {
            a.cfbar[(size_t)sc * N3 + 3 * i + c] = fb[3 * i + c];
            // f_app = diag copies (:669-671)
            if (wt) st_wt(a.fdes + (size_t)sc * N3 + 3 * i + c, myf[3 * i + c]);
            else a.fdes[(size_t)sc * N3 + 3 * i + c] = myf[3 * i + c];
          }
          a.qstatus[(size_t)sc * n + i] = qstat;
          if (i == 0) {
            if (wt) {
              st_wt(a.iters + sc, iter);
              st_wt(a.ipmx + sc, L.wmx[ls]);
            } else {
              a.iters[sc] = iter;
              a.ipmx[sc] = L.wmx[ls];
            }
          }
        }
        if (wt) {
          // the stamp follows the wavefront's stores (all the scenario's lanes are in this wavefront).  No fence:
          // the bytes above left the L2 with their stores
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (i == 0 && vi == 0) st_wt(a.done + sc, a.serial);
        }
        if (kstep + 1 < a.ksteps) {
          // fused steps: the scenario's next control step in the same slot (warm f, f_mean, lambda kept;
          // rho and the iteration count restart as in a new control call, control/rqp_cadmm.py:631-640)
          ++kstep;
          prev_iter = iter;
          iter = 0;
          qstat = ST_OPTIMAL;
          rho = a.rho0;
          if (RB) wrl[0] = 0.0;
          rebuild = true;  // (the shared data of the step: at the top of the next pass)
          if (i == 0 && vi == 0) L.wmx[ls] = 0;
        } else if (i == 0) {
          L.sid[ls] = -1;
        }
      }
    }
    __syncthreads();
  }
  // work counters of this class: one atomic per wavefront
  unsigned long long* const cc = a.counters + CNT_STRIDE * CLS;
  flush_solve_counters(a, cc, wc);
  const unsigned long long ce = RB ? wave_sum(wc.cert) : 0, sx = RB ? wave_sum(wc.stall) : 0;
  const unsigned long long wm = RB ? wave_sum(wc.warm) : 0;
  if (lane == 0) {
    if (RB) {  // the tail's occupancy apart from k_cadmm's class counters
      unsigned long long* ct = a.counters + CNT_TAIL;
      atomicAdd(ct, (unsigned long long)wc.pass);
      atomicAdd(ct + 1, (unsigned long long)wc.slot);
      if (ce) atomicAdd(ct + 3, ce);
      if (sx) atomicAdd(ct + 4, sx);
      if (wm) atomicAdd(ct + 5, wm);
    } else {
      atomicAdd(cc + 3, (unsigned long long)(wc.slot * NT));
      atomicAdd(cc + 4, (unsigned long long)(wc.pass * G));
    }
  }
  __syncthreads();
}

// The C-ADMM control step of every scenario: persistent blocks drain the env classes in order of
// decreasing row count (the longest-running scenarios first), each class with its own row-slot
// instantiation of the IPM.  All wavefronts work on the same class at (nearly) the same time: the
// unrolled IPM of one class is ~80-130 KB of code, and wavefronts of different classes sharing a
// CU's instruction cache measured 16 % slower (proportional class starts: 12.9 vs 11.1 ms, C4 path).
// RMS: the row modes of classes 0 .. 2 (rm_pack); the host launches the instantiation of the launch's word.
template <bool ADV, int RMS>
__global__ __launch_bounds__(64) void k_cadmm(KArgs a) {
  cadmm_drain<3, false, ADV, 0>(a);
  cadmm_drain<2, false, ADV, rm_of(RMS, 2)>(a);
  cadmm_drain<1, false, ADV, rm_of(RMS, 1)>(a);
  cadmm_drain<0, false, ADV, rm_of(RMS, 0)>(a);
}
// Without a forest every scenario is in env class 0 (k_env_class finds no tree): the class-0 drain in a
// kernel of its own, with a 960 B/lane scratch frame instead of k_cadmm's 1,728 (same arithmetic).  C5
// 84.2 / 84.1 -> 80.3 / 79.9 ms per step, C2 12.7 / 12.9 -> 12.0 / 12.1 (round 4, kernel-trace A/B).
// With a forest one launch per class measured 2x slower on C4 (each class launch drains to its own
// tail): k_cadmm keeps the four drains in one launch there.
template <bool ADV, int RM0>
__global__ __launch_bounds__(64) void k_cadmm0(KArgs a) { cadmm_drain<0, false, ADV, RM0>(a); }

// The launch of a unit's drain kernels (ADV: the unit's): the instantiation of the word rms, one per word of
// DAT_CADMM_RMS -- k_cadmm0 by class 0's mode alone.  A word that is not built is refused (dat_create and
// dat_debug_row_modes refuse it before: cadmm_rms_built).
template <bool ADV>
inline hipError_t launch_k_cadmm_of(bool forest, int rms, int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  void (*k)(KArgs) = nullptr;
#define DAT_X(m0, m1, m2) \
  if (rms == rm_pack(m0, m1, m2)) k = forest ? k_cadmm<ADV, rm_pack(m0, m1, m2)> : k_cadmm0<ADV, m0>;
  DAT_CADMM_RMS(DAT_X)
#undef DAT_X
  if (!k) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k, dim3(blocks), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace
