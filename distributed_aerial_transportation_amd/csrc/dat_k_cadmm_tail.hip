// dat_k_cadmm_tail.hip -- the C-ADMM tail kernels, k_cadmm_tail and k_cadmm0_tail (cadmm_drain<., true, false>,
// dat_cadmm_drain.hpp), their dynamic-LDS limit, and k_agent_qp, the raw batched agent QPs: the kernels that carry
// the robust solver.  Two fifths of the library's device code, in a unit of its own (dat_launch.hpp: the units, and
// why k_agent_qp is here).
#include <hip/hip_runtime.h>

#include <cmath>
#include <initializer_list>
#include <mutex>

#include "dat_cadmm_drain.hpp"
#include "dat_dd_step.hpp"
#include "dat_launch.hpp"

namespace {

// The tail: the scenario-steps k_cadmm handed over (an agent QP not clean, or the tail rule) and, launched
// concurrently with k_cadmm, those k_env_class routed here (wedged in a stall), one scenario per wavefront,
// every class's row state and IPM aux slots in LDS: the robust redo, the certificate of infeasible rows, the warm
// start and stall exit of the tail rule's passes.  A kernel of its own: the robust solver compiled into k_cadmm
// cost the fast path 36-60 % (register allocation, C4 A/B).  Without a listed scenario its blocks return at once.
__global__ __launch_bounds__(64) void k_cadmm_tail(KArgs a) {
  cadmm_drain<3, true, false, 3>(a);
  cadmm_drain<2, true, false, 3>(a);
  cadmm_drain<1, true, false, 3>(a);
  cadmm_drain<0, true, false, 3>(a);
}
// (without a forest: the class-0 drain alone, as k_cadmm0)
__global__ __launch_bounds__(64) void k_cadmm0_tail(KArgs a) { cadmm_drain<0, true, false, 3>(a); }

// the kernel's argument type, named as it was when the kernel got its symbol: dat::AgentQPArgs's fields
struct AgentQPArgs : dat::AgentQPArgs {
  AgentQPArgs(const dat::AgentQPArgs& q) : dat::AgentQPArgs(q) {}
};

// ------------------------------------------------------------------------------------------------
// raw batched agent QPs: RQPPrimalSolver.solve (control/rqp_cadmm.py:482-501, control/rqp_dd.py:475-505)
// ------------------------------------------------------------------------------------------------
// One lane per item (a scenario's state / parameters / forest, one agent, its own multipliers).
// Not a hot path: the scenario data live in lane registers / scratch (PlainRef), as in k_cent.
__global__ __launch_bounds__(64) void k_agent_qp(KArgs a, AgentQPArgs q) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = k < q.count;
  const int n = a.n, N3 = 3 * n;
  const bool dd = a.dlamF != nullptr;
  const int sc = valid ? q.scen[k] : 0, i = valid ? q.agent[k] : 0;
  const double* prm = prm_of(a, sc);
  const double* st = a.state + (size_t)sc * a.S;
  QPShared S;
  QPLane<1> P;
  EnvRows E;
  double Rt_all[NMAX * 9];
  int nr = NBASE;
  EnvOut env;
  env.collision = 0;
  env.min_env_dist = 0.0;
  if (valid) {
    for (int j = 0; j < n; ++j) make_Rt(prm + DAT_P_RCOM(n) + 3 * j, st + DAT_S_RL(n), Rt_all + 9 * j);
    build_shared(S, prm, n, st, q.acc + (size_t)k * 6, prm[DAT_P_KFD], prm[DAT_P_KMD], 3, !dd);
    if (dd) {
      lane_dd_static(P, prm, i);
    } else {
      lane_cadmm_static(P, prm, i);
    }
    const double* trees;
    int nt;
    unsigned emask;
    double lhs[DAT_NENV][3], rhs[DAT_NENV];
    if (q.elhs) {
      // the caller's rows, compacted (slots 0 .. nenv - 1); no env query: no collision, distance +inf
      emask =
          env_slots_of_rows(q.elhs + (size_t)k * DAT_NENV * 3, q.erhs + (size_t)k * DAT_NENV, q.nenv[k], lhs, rhs);
      env.min_env_dist = INFINITY;
    } else {
      forest_of(a, sc, &trees, &nt);
      env = env_rows(prm, n, st, trees, nt, i, prm[DAT_P_AENVD], &emask, lhs, rhs);
    }
    set_env_rows(P, E, S, emask, lhs, rhs);
    nr = rows_needed(P.emask);
    if (dd) {
      set_dd_price(P, prm, n, i, q.c9 + (size_t)k * 9);
    } else {
      lane_cadmm_dynamic(P, prm, n, i, Rt_all, q.lam + (size_t)k * N3, q.fbar + (size_t)k * N3, q.rho[k]);
    }
  }
  nr = wave_max(nr);
  if (!valid) return;
  double y[1][3], w[6];
  const PlainRef<QPShared> shr{&S};
  const EnvPlain er{&E};
  const RtPtr rtr{Rt_all + 9 * i};
  double* bst = q.best + (size_t)k * best_size(1);
  // the C-ADMM agent QP as the closed loop solves it: rows certified infeasible are held (k_cadmm_tail)
  const bool cert = !dd && cadmm_certify_rows(P, shr, er);
  IPMOut o = dd ? ipm_solve_rows<MODE_DD, 1>(nr, shr, er, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst, IPM_MAX_ITER,
                                             a.qp_tol)
                : ipm_solve_rows<MODE_CADMM, 1, IPM_FAST_REDO>(nr, shr, er, rtr, P, prm + DAT_P_FEQ(n) + 3 * i, y, w, bst,
                                                IPM_MAX_ITER, a.qp_tol);
  if (dd) {
    double* xo = q.x + (size_t)k * 9;
    for (int c = 0; c < 3; ++c) xo[c] = y[0][c];
    for (int c = 0; c < 6; ++c) xo[3 + c] = w[c];
  } else {
    double* xo = q.x + (size_t)k * N3;
    cadmm_copy_of_solve(xo, y[0], o.pi, Rt_all, 9, q.lam + (size_t)k * N3, q.fbar + (size_t)k * N3, q.rho[k], n, i);
  }
  // in-band accepts (rare: per lane, no wavefront reduction)
  if (o.inband) atomicAdd(a.counters + CNT_INBAND, 1);
  if (inband_loose(o)) atomicAdd(a.counters + CNT_INBAND + 1, 1);
  atomicAdd(a.counters + CNT_REF, (unsigned long long)o.refs);
  atomicAdd(a.counters + CNT_REF + 1, (unsigned long long)o.corrs);
  q.status[k] = o.status;
  q.iters[k] = o.iters;
  q.col[k] = (unsigned char)env.collision;
  q.mind[k] = env.min_env_dist;
  q.cert[k] = (unsigned char)cert;
}

}  // namespace

namespace dat {

hipError_t launch_k_cadmm_tail(bool forest, int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  hipLaunchKernelGGL(forest ? k_cadmm_tail : k_cadmm0_tail, dim3(blocks), dim3(64), lds, st, a);
  return hipGetLastError();
}

// the tail's workgroup may exceed the default 64 KB of dynamic LDS
hipError_t tail_lds_limit_raise(int device, int n) {
  // The limit belongs to the kernel (per device), not to the handle: it is only ever raised, so a handle
  // of a smaller team created later never lowers it under a live handle of a larger one.
  static std::mutex mu;
  static int cur[64] = {0};
  const int tl = (int)cadmm_tail_lds_bytes(n);
  std::lock_guard<std::mutex> lk(mu);
  int* have = device >= 0 && device < 64 ? &cur[device] : nullptr;
  if (!have || tl > *have) {
    for (const void* k : {(const void*)k_cadmm_tail, (const void*)k_cadmm0_tail})
      if (const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, tl); e != hipSuccess)
        return e;
    if (have) *have = tl;
  }
  return hipSuccess;
}

hipError_t launch_k_agent_qp(hipStream_t st, const KArgs& a, const AgentQPArgs& q) {
  hipLaunchKernelGGL(k_agent_qp, dim3((q.count + 63) / 64), dim3(64), 0, st, a, q);
  return hipGetLastError();
}

}  // namespace dat
