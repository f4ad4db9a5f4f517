// dat_dd_drain.hpp -- the DD control step's kernel template k_dd<ENV> and the LDS carve it and the host's launch go
// by.  Instantiated beside the C-ADMM drains (ENV = false: dat_k_cadmm.hip, ENV = true: dat_k_cadmm_adv.hip), not in
// a unit of its own: dat_launch.hpp says why (build_shared).
#pragma once

#include "dat_dd_step.hpp"
#include "dat_drain_common.hpp"

// Internal linkage, as in the one unit this text came from: each unit's inliner weighs these functions as it did
// there, and a kernel keeps its symbol.
namespace {
using namespace dat;

// ------------------------------------------------------------------------------------------------
// DD step
// ------------------------------------------------------------------------------------------------
constexpr int DD_ES = 7, DD_RS = 5;
// k_dd per-wavefront area: with a forest the env rows' LDS image; without one nothing (n = 6:
// 27.0 KB, four wavefronts per CU -- the unused 20 KB image used to hold k_dd at three, C3 A/B
// 23.8 -> 22.7 ms).  The 3 base rows' IPM state stays in registers: RowLds measured 26.2 ms, and rows
// (+ aux slots) in LDS without a forest measured no gain on C3 in round 3 (git history).
__host__ __device__ constexpr int dd_area_doubles(bool env) { return env ? ENV_LDS_DOUBLES : 0; }
constexpr int DD_SLOT_INTS = 64;  // ints of each per-slot array of k_dd (G <= 21 used)
// dynamic LDS of a k_dd workgroup of G = floor(64/n) scenario slots (NT = G n lanes): as DdSetupLds
struct DdLds {
  double *X, *lamF, *lamM, *E, *Rts, *red, *envs;
  QPShared* shs;
  int *sid, *done, *wmx, *lng, *end;
  size_t bytes() const { return (size_t)((char*)end - (char*)X); }
};
__host__ __device__ inline DdLds dd_carve(double* smem, int n, bool env) {
  const int N3 = 3 * n, G = 64 / n, NT = G * n;
  DdLds L;
  L.X = smem;                                       // NT x 9   (f_i, F_i, M_i)
  L.lamF = L.X + al2(NT * 9);                       // G x 3n
  L.lamM = L.lamF + al2(G * N3);                    // G x 3n
  L.E = L.lamM + al2(G * N3);                       // NT x ES  consensus error (ES = 7: odd stride, no bank conflicts)
  L.Rts = L.E + al2(NT * DD_ES);                    // G x n x RT_STRIDE
  L.red = L.Rts + G * RT_STRIDE * n;                // 64 x DD_RS
  L.shs = (QPShared*)(L.red + 64 * DD_RS);          // G
  L.envs = (double*)(L.shs + G);                    // EnvLds image (env only)
  L.sid = (int*)(L.envs + dd_area_doubles(env));    // G: scenario of the slot (-1 empty, -2 retired)
  L.done = L.sid + DD_SLOT_INTS;                    // G: the slot's scenario stopped in this pass
  L.wmx = L.done + DD_SLOT_INTS;                    // G: IPM iterations of the slot's slowest agent QP this step
  L.lng = L.wmx + DD_SLOT_INTS;                     // G: the slot's chain is a long one (dd_long_chain)
  L.end = L.lng + DD_SLOT_INTS;
  return L;
}

// DD control step (control/rqp_dd.py:695-752), persistent: each 64-lane block holds G = floor(64/n)
// scenario slots of n lanes (one lane per agent QP) and drains the sorted scenario queue; a slot whose
// scenario stops is refilled at the next dual-ascent pass.  A scenario's arithmetic does not depend
// on the slot or block that runs it.  ENV = false (no forest on the handle): every QP has the three
// base rows only, and the IPM is instantiated for them alone (the register footprint of the 13-slot
// instantiation is not paid).
template <bool ENV>
__global__ __launch_bounds__(64) void k_dd(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int n = a.n, N3 = 3 * n, N6 = 6 * n;
  const int G = 64 / n, NT = G * n;
  const int lane = threadIdx.x;
  const int ls = lane / n, i = lane - ls * n;
  const int lsc = ls < G ? ls : 0;
  const DdLds L = dd_carve(smem, n, ENV);
  QPShared& S = L.shs[lsc];
  double* myX = L.X + lane * 9;
  const double* Xs = L.X + lsc * n * 9;  // the slot's agent records (dat_dd_step.hpp)
  const double* Es = L.E + lsc * n * DD_ES;
  double* lF = L.lamF + lsc * N3;
  double* lM = L.lamM + lsc * N3;
  double* rts = L.Rts + lsc * RT_STRIDE * n;
  const int cnt = a.scount[sc_at(SC_SIZE, 0)], first = a.scount[sc_at(SC_START, 0)];
  const LdsRef<QPShared> shr{L.shs, lsc};
  const EnvLds err{L.envs, lane};
  const RtLds rtr{L.Rts, (lsc * n + i) * RT_STRIDE};
  if (lane < G) L.sid[lane] = -1;
  __syncthreads();

  QPLane<1> P;
  const double* prm = nullptr;
  const double* Rl = nullptr;
  double* bst = nullptr;
  double* wrl = nullptr;  // the agent QP's warm-start record (HBM)
  double prev[9];
  int sc = -1, iter = 0, qstat = ST_OPTIMAL, col = 0;
  int kstep = 0;  // fused control steps (dat_control_steps): the slot scenario's current step
  double mdist = 0.0;
  WaveCounters wc;
  // phase marks (DAT_PHASE_PROF builds, tools/phase_prof.py): 11 refill + fresh slot setup, 14 prices,
  // 10 ipm_solve, 9 result bookkeeping, 13 consensus error, stop test, dual ascent, outputs
  DAT_PHASE_INIT(11);
  for (;;) {
    DAT_PHASE(11);
    // ---- refill empty slots from the queue
    if (lane < NT && i == 0 && L.sid[ls] == -1) {
      const int q = atomicAdd(a.scount + sc_at(SC_HEAD, 0), 1);
      L.sid[ls] = q < cnt ? a.slist[first + q] : -2;
      L.done[ls] = 0;
      L.wmx[ls] = 0;
      L.lng[ls] = 0;
    }
    __syncthreads();
    const int slot_sc = lane < NT ? L.sid[ls] : -2;
    const bool fresh = slot_sc >= 0 && slot_sc != sc;
    if (fresh) {
      sc = slot_sc;
      prm = prm_of(a, sc);
      const double* st = a.state + (size_t)sc * a.S;
      Rl = st + DAT_S_RL(n);
      make_Rt(prm + DAT_P_RCOM(n) + 3 * i, Rl, rts + RT_STRIDE * i);
      for (int c = 0; c < 3; ++c) {
        lF[3 * i + c] = a.dlamF[(size_t)sc * N3 + 3 * i + c];
        lM[3 * i + c] = a.dlamM[(size_t)sc * N3 + 3 * i + c];
      }
      for (int c = 0; c < 9; ++c) prev[c] = a.dprev[((size_t)sc * n + i) * 9 + c];
      for (int c = 0; c < 9; ++c) myX[c] = prev[c];  // the controller's current (f, F, M)
      bst = a.best + ((size_t)sc * n + i) * BEST_REC;
      wrl = a.wrec + ((size_t)sc * n + i) * WREC_SIZE;
      wrl[0] = 0.0;
      iter = 0;
      qstat = ST_OPTIMAL;
      kstep = 0;
      if (i == 0) build_shared(S, prm, n, st, a.acc + (size_t)sc * 6, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, false);
    }
    if (!__syncthreads_or(slot_sc >= 0)) break;  // every slot retired
    if (fresh) {
      lane_dd_static(P, prm, i);
      col = 0;
      mdist = prm[DAT_P_VISR];
      if (ENV) {
        const double* trees;
        int nt;
        unsigned emask;
        forest_of(a, sc, &trees, &nt);
        double lhs[DAT_NENV][3], rhs[DAT_NENV];
        EnvOut env = env_rows(prm, n, a.state + (size_t)sc * a.S, trees, nt, i, prm[DAT_P_AENVD], &emask, lhs, rhs);
        col = env.collision;
        mdist = env.min_env_dist;
        EnvRows Ev;
        set_env_rows(P, Ev, S, emask, lhs, rhs);
        env_to_lds(L.envs, lane, Ev);
      }
    }
    const bool active = slot_sc >= 0;
    const int nr = wave_max(active ? rows_needed(P.emask) : NBASE);
    DAT_PHASE(14);
    if (active) {
      double c9[9];
      dd_prices(prm, n, i, lF, lM, Rl, c9);
      set_dd_price(P, prm, n, i, c9);
      double y[1][3], w[6];
      IPMOut o;
      const double* y0 = prm + DAT_P_FEQ(n) + 3 * i;
      DAT_PHASE(10);
      // a late pass of a long chain: the agent QP differs from the previous pass's only in its prices, so it starts
      // from that pass's last iterate (ipm_solve WS, the tail kernel's warm start); a long chain's QPs are solved
      // tighter (dd_qp_tol, dat_dd_step.hpp)
      const bool lng = L.lng[ls] != 0;
      const bool wson = dd_warm_start(iter, lng);
      const double qtol = dd_qp_tol(lng, a.qp_tol);
      if constexpr (ENV)
        o = ipm_solve_rows<MODE_DD, 1, IPM_FAST, true>(nr, shr, err, rtr, P, y0, y, w, bst, IPM_MAX_ITER, qtol, wrl,
                                                       wson);
      else
        o = ipm_solve<MODE_DD, 1, NBASE, LdsRef<QPShared>, EnvLds, RtLds, RowRegs, 0, NoGrp, IPM_FAST, true>(
            shr, err, rtr, P, y0, y, w, bst, IPM_MAX_ITER, qtol, RowRegs{}, NoGrp{}, wrl, wson);
      DAT_PHASE(9);
      wc.ipm += o.iters;
      wc.inband += o.inband;
      wc.loose += inband_loose(o);
      wc.refs += o.refs;
      wc.corrs += o.corrs;
      atomicMax(&L.wmx[ls], o.iters);
#ifdef DAT_ITER_HIST
      atomicAdd(&g_iter_hist[o.iters < 63 ? o.iters : 63], 1ull);
#endif
      wc.rowit += (long long)o.iters * (__builtin_popcount(S.bmask) + __builtin_popcount(P.emask));
      ++wc.qp;
      qstat = o.status;
      dd_take_solve(o.status, y[0], w, prm, n, i, Xs, prev);
    }
    DAT_PHASE(13);
    __syncthreads();  // agent 0's fallback above reads X before this pass's writes
    if (active) {
      for (int c = 0; c < 9; ++c) myX[c] = prev[c];
    }
    __syncthreads();
    if (active) {
      ++iter;
      dd_consensus_error(Xs, rts, RT_STRIDE, n, i, L.E + lane * DD_ES);
      L.red[lane * DD_RS + 0] = col ? 1.0 : 0.0;
      L.red[lane * DD_RS + 1] = mdist;
    }
    __syncthreads();
    if (active && i == 0) {
      const double res = dd_pass_residual(Es, DD_ES, n);
      const bool stop = dd_stop(res, a.res_tol, iter, a.max_iter);
      if (!stop && a.record_err && a.err) a.err[(size_t)sc * (a.max_iter + 1) + iter - 1] = res;
      L.done[ls] = stop ? 1 : 0;
      if (!stop && dd_long_chain(iter, res)) L.lng[ls] = 1;
    }
    __syncthreads();
    if (active) {
      if (!L.done[ls]) {
        dd_dual_ascent(a.dHinv + (size_t)sc * N6 * N6 + (size_t)(6 * i) * N6, N6, Es, DD_ES, n, lF + 3 * i, lM + 3 * i);
      } else {
        // the scenario stopped: write its outputs and free the slot
        for (int c = 0; c < 3; ++c) {
          a.dlamF[(size_t)sc * N3 + 3 * i + c] = lF[3 * i + c];
          a.dlamM[(size_t)sc * N3 + 3 * i + c] = lM[3 * i + c];
          a.fdes[(size_t)sc * N3 + 3 * i + c] = myX[c];
        }
        for (int c = 0; c < 9; ++c) a.dprev[((size_t)sc * n + i) * 9 + c] = prev[c];
        a.qstatus[(size_t)sc * n + i] = qstat;
        if (i == 0) {
          a.iters[sc] = iter;
          a.ipmx[sc] = L.wmx[ls];
          int coll = 0;
          double md = prm[DAT_P_VISR];
          for (int k = 0; k < n; ++k) {
            coll |= L.red[(ls * n + k) * DD_RS] != 0.0;
            md = fmin(md, L.red[(ls * n + k) * DD_RS + 1]);
          }
          a.col[sc] = (unsigned char)coll;
          a.mind[sc] = md;
        }
        if (kstep + 1 < a.ksteps) {
          // fused steps (no forest): the scenario's next control step in the same slot, from the warm
          // lambda_F, lambda_M and previous solutions it leaves (control/rqp_dd.py:695-700)
          ++kstep;
          iter = 0;
          wrl[0] = 0.0;
          qstat = ST_OPTIMAL;
          if (i == 0) {
            build_shared(S, prm, n, a.state + (size_t)sc * a.S, a.acc + ((size_t)kstep * a.B + sc) * 6,
                         prm[DAT_P_KFD], prm[DAT_P_KMD], 3, false);
            L.wmx[ls] = 0;
            L.lng[ls] = 0;
          }
        } else if (i == 0) {
          L.sid[ls] = -1;
        }
      }
    }
    __syncthreads();
  }
  flush_solve_counters(a, a.counters, wc);
}

}  // namespace
