// dat_drain_common.hpp -- what the persistent drains share (cadmm_drain, dat_cadmm_drain.hpp; k_dd, dat_k_dd.hip):
// the LDS carves' alignment and the wavefront's work counters.
#pragma once

#include "dat_kargs.hpp"

// Internal linkage, as in the one unit this text came from: each unit's inliner weighs these functions as it did
// there, and a kernel keeps its symbol.
namespace {
using namespace dat;

// doubles rounded up to a 16-byte multiple: every LDS region starts 16-byte aligned (pair reads)
__host__ __device__ constexpr size_t al2(size_t d) { return (d + 1) & ~(size_t)1; }

// Work counters of one wavefront, flushed once per class it drained.
struct WaveCounters {
  long long qp = 0, ipm = 0, rowit = 0;  // lane-level: agent-QP solves, IPM iterations, x active rows
  long long inband = 0, loose = 0;      // lane-level: solves accepted through the best in-band iterate
  long long refs = 0, corrs = 0;        // lane-level: IPM refinement passes, corrections applied
  long long slot = 0, pass = 0;         // wave-level: sum of (max lane IPM iterations) per pass, passes
  long long cert = 0, stall = 0, warm = 0;  // k_cadmm_tail, lane-level: certified infeasible, stall exits, warm starts
};
// wave-uniform sum (every lane of the wavefront must execute it)
__device__ inline unsigned long long wave_sum(long long v) {
  unsigned long long s = (unsigned long long)v;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}
// The lane-level solve counters of a wavefront (C-ADMM drain, k_dd), one atomic each: agent-QP solves, IPM
// iterations and x active rows to cc[0 .. 2] (the class's counters), in-band accepts and refinement work to
// CNT_INBAND / CNT_REF.  Every lane of the wavefront must execute it.
__device__ __forceinline__ void flush_solve_counters(const KArgs& a, unsigned long long* cc, const WaveCounters& wc) {
  const unsigned long long q = wave_sum(wc.qp), ip = wave_sum(wc.ipm), rw = wave_sum(wc.rowit);
  const unsigned long long ib = wave_sum(wc.inband), lo = wave_sum(wc.loose);
  const unsigned long long rf = wave_sum(wc.refs), co = wave_sum(wc.corrs);
  if (threadIdx.x == 0) {
    atomicAdd(cc, q);
    atomicAdd(cc + 1, ip);
    atomicAdd(cc + 2, rw);
    if (ib) atomicAdd(a.counters + CNT_INBAND, ib);
    if (lo) atomicAdd(a.counters + CNT_INBAND + 1, lo);
    atomicAdd(a.counters + CNT_REF, rf);
    atomicAdd(a.counters + CNT_REF + 1, co);
  }
}

}  // namespace
