// dat_k_dd.hip -- the DD kernels before the drain: k_dd_setup<0, 3..8> (the quasi-Newton matrix) and k_dd_key (the
// drain order), and the byte counts of the DD carves for the host's launches.  A unit of its own (dat_launch.hpp);
// k_dd<ENV> itself is dat_dd_drain.hpp, instantiated beside the C-ADMM drains.
#include <hip/hip_runtime.h>

#include "dat_dd_drain.hpp"
#include "dat_launch.hpp"

using namespace dat;

namespace {

// ------------------------------------------------------------------------------------------------
// DD: quasi-Newton matrix inverse per scenario (one 64-lane block per scenario)
// ------------------------------------------------------------------------------------------------
// Q_i (strong_convexity_matrix), the eliminations' per-element steps and the H element: dat_dd_step.hpp
// k_dd_setup keeps the columns of [H | I] in registers for n <= DD_REG_NMAX (dd_setup_h_regs), in LDS
// beyond
constexpr int DD_REG_NMAX = 8;
// doubles of the [H | I] area of k_dd_setup; it first holds the per-agent [Q_i | I] (162 n), their
// pivot columns (9 n) and pivot rows (n ints).  Register path: the Q_i area and two N-double pivot
// column buffers only.
__host__ __device__ inline int dd_setup_hs(int n) {
  const int N = 6 * n;
  if (n <= DD_REG_NMAX) return 171 * n + 1 + 2 * N;  // k_dd_setup<n>
  return 2 * N * N > 171 * n + 1 ? 2 * N * N : 171 * n + 1;
}
// dynamic LDS of a k_dd_setup workgroup: the kernel's regions in order and their end.  The kernel carves its smem;
// the host carves from a null base and reads the launch's bytes, so the layout is stated once.
struct DdSetupLds {
  double *Qi, *Rts, *H, *fac, *end;
  size_t bytes() const { return (size_t)((char*)end - (char*)Qi); }
};
__host__ __device__ inline DdSetupLds dd_setup_carve(double* smem, int n) {
  DdSetupLds L;
  L.Qi = smem;                       // n x 81   sym(Q_i^-1)
  L.Rts = L.Qi + 81 * n;             // n x 9
  L.H = L.Rts + 9 * n;               // N x 2N   [H | I]
  L.fac = L.H + dd_setup_hs(n);      // N
  L.end = L.fac + 6 * n;
  return L;
}

// H = A blkdiag(Q_j^-1) A' (control/rqp_dd.py:642-655) and H^-1 by Gauss-Jordan on [H | I], n = NB,
// with the columns of [H | I] in registers: lane c owns column c and, when 2N > 64, column c + 64 (an
// identity column: N <= 48).  Same per-element arithmetic and order as the LDS path, so the result is
// bitwise equal: H_rc summed over blocks j, then over the support p of row r's block in increasing
// order, of A_rp (Q_j A_c)_p with (Q_j A_c)_p summed over q in increasing order; Gauss-Jordan without
// pivoting (H is SPD), per element hk = h_kc / piv, h_rc -= f_r hk.  The column is kept rotated so
// that step k's pivot row is element 0 (no runtime register index): the owner of column k publishes it
// in LDS (double buffered), every lane updates its columns and rotates them by one.
// The elimination's element steps are the header's (dd_hinv_scale, dd_hinv_eliminate).  The assembly restates
// dd_arow / dd_h_element by the row's three cases: here the row r is a compile-time index and the column's agent
// and component are the lane's, so the header's form (a 9-vector per row, zeros skipped by value) would run the
// sums over runtime zeros and index registers at run time.
template <int NB>
__device__ void dd_setup_h_regs(const KArgs& a, int sc, const double* Qi, const double* Rts, double* fac) {
  constexpr int N = 6 * NB;
  constexpr bool TWO = 2 * N > 64;
  const int lane = threadIdx.x;
  double h[N], g[TWO ? N : 1];
  // ---- assembly of column lane (H columns for lane < N, identity columns e_{lane - N} beyond)
#pragma unroll
  for (int r = 0; r < N; ++r) {
    h[r] = (lane >= N && r == lane - N) ? 1.0 : 0.0;
    if (TWO) g[r] = (r == lane + 64 - N) ? 1.0 : 0.0;
  }
  if (lane < N) {
    const int ag = lane / 6, comp = lane - 6 * ag;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const double* Q = Qi + 81 * j;
      // w = Q_j a_{c,j}: a_{c,j} = e_{3+comp} (j == ag), -e_comp (comp < 3), -Rt_j[comp-3, :] on f_j
      double w[9];
      if (j == ag) {
#pragma unroll
        for (int p = 0; p < 9; ++p) { double t = 0.0; t += Q[9 * p + 3 + comp] * 1.0; w[p] = t; }
      } else if (comp < 3) {
#pragma unroll
        for (int p = 0; p < 9; ++p) { double t = 0.0; t += Q[9 * p + comp] * -1.0; w[p] = t; }
      } else {
        const double* rt = Rts + 9 * j + 3 * (comp - 3);
        const double v0 = -rt[0], v1 = -rt[1], v2 = -rt[2];
#pragma unroll
        for (int p = 0; p < 9; ++p) {
          double t = 0.0;
          t += Q[9 * p] * v0;
          t += Q[9 * p + 1] * v1;
          t += Q[9 * p + 2] * v2;
          w[p] = t;
        }
      }
#pragma unroll
      for (int r = 0; r < N; ++r) {
        const int agr = r / 6, cr = r % 6;
        if (j == agr) {
          h[r] += 1.0 * w[3 + cr];
        } else if (cr < 3) {
          h[r] += -1.0 * w[cr];
        } else {
          const double* rt = Rts + 9 * j + 3 * (cr - 3);
          h[r] += -rt[0] * w[0];
          h[r] += -rt[1] * w[1];
          h[r] += -rt[2] * w[2];
        }
      }
    }
  }
  // ---- Gauss-Jordan, columns rotated (h[i] = [H | I]_{(k + i) mod N, c} at step k)
  for (int k = 0; k < N; ++k) {
    double* f = fac + (k & 1) * N;
    if (lane == k) {
#pragma unroll
      for (int i = 0; i < N; ++i) f[i] = h[i];
    }
    __syncthreads();
    const double piv = f[0];
    {
      const double hk = dd_hinv_scale(h[0], piv);
#pragma unroll
      for (int i = 1; i < N; ++i) dd_hinv_eliminate(h[i], f[i], hk);
#pragma unroll
      for (int i = 0; i < N - 1; ++i) h[i] = h[i + 1];
      h[N - 1] = hk;
    }
    if (TWO) {
      const double hk = dd_hinv_scale(g[0], piv);
#pragma unroll
      for (int i = 1; i < N; ++i) dd_hinv_eliminate(g[i], f[i], hk);
#pragma unroll
      for (int i = 0; i < N - 1; ++i) g[i] = g[i + 1];
      g[N - 1] = hk;
    }
  }
  // ---- H^-1 = the right half: column N + c' of [H | I] is column c' of H^-1 (row-major output)
  double* out = a.dHinv + (size_t)sc * N * N;
  if (lane >= N && lane < 2 * N) {
#pragma unroll
    for (int r = 0; r < N; ++r) out[(size_t)r * N + (lane - N)] = h[r];
  }
  if (TWO && lane + 64 < 2 * N) {
#pragma unroll
    for (int r = 0; r < N; ++r) out[(size_t)r * N + (lane + 64 - N)] = g[r];
  }
}

// NB = n (<= DD_REG_NMAX: H columns in registers, one instantiation per team size so each has its own
// register footprint) or 0 (any n: H in LDS)
template <int NB>
__global__ __launch_bounds__(64) void k_dd_setup(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int n = a.n, N = 6 * n;
  const int sc = blockIdx.x;
  const int lane = threadIdx.x;
  if (sc >= a.B) return;
  const DdSetupLds L = dd_setup_carve(smem, n);
  const double* prm = prm_of(a, sc);
  const double* st = a.state + (size_t)sc * a.S;
  // Q_i^-1 by Gauss-Jordan with partial pivoting (np.linalg.inv) on [Q_i | I] in LDS, spread over
  // the wavefront: lane pairs (agent j, column c) update one column each, with the per-element
  // arithmetic of the serial elimination (pivot column copied before the update).
  double* Aug = L.H;                       // n x 9 x 18, in the [H | I] area (built afterwards)
  double* colk = Aug + 162 * n;            // n x 9: column k before step k's update
  int* pivr = (int*)(colk + 9 * n);        // n
  if (lane < n) {
    double Q[81];
    dd_strong_convexity(prm, n, st, lane, Q);
    dd_qinv_augment(Q, Aug + 162 * lane);
    make_Rt(prm + DAT_P_RCOM(n) + 3 * lane, st + DAT_S_RL(n), L.Rts + 9 * lane);
  }
  __syncthreads();
  for (int k = 0; k < 9; ++k) {
    if (lane < n) pivr[lane] = dd_qinv_pivot_row(Aug + 162 * lane, k);
    __syncthreads();
    for (int e = lane; e < 18 * n; e += 64) {  // row exchange k <-> p, column by column
      const int j = e / 18, c = e - 18 * j;
      dd_qinv_exchange(Aug + 162 * j, k, pivr[j], c);
    }
    __syncthreads();
    for (int e = lane; e < 9 * n; e += 64) {
      const int j = e / 9, r = e - 9 * j;
      colk[e] = Aug[162 * j + 18 * r + k];
    }
    __syncthreads();
    for (int e = lane; e < 18 * n; e += 64) {
      const int j = e / 18, c = e - 18 * j;
      dd_qinv_update_col(Aug + 162 * j, colk + 9 * j, k, c);
    }
    __syncthreads();
  }
  for (int e = lane; e < 81 * n; e += 64) {
    const int j = e / 81, rc = e - 81 * j, r = rc / 9, c = rc - 9 * r;
    L.Qi[e] = dd_qinv_sym(Aug + 162 * j, r, c);
  }
  __syncthreads();
  if constexpr (NB > 0) {
    dd_setup_h_regs<NB>(a, sc, L.Qi, L.Rts, L.H + 171 * n + 1);  // pivot columns past the Q_i elimination area
    return;
  }
  // H = A blkdiag(Q_j^-1) A'  (control/rqp_dd.py:642-655)
  for (int e = lane; e < N * N; e += 64) {
    int r = e / N, c = e % N;
    L.H[2 * N * r + c] = dd_h_element(L.Qi, L.Rts, n, r, c);
    L.H[2 * N * r + N + c] = (r == c) ? 1.0 : 0.0;
  }
  __syncthreads();
  // Gauss-Jordan on [H | I] (H is SPD: no pivoting needed)
  // Each lane owns whole columns of [H | I] (no index division; a row of the tile is contiguous
  // across lanes, so the LDS accesses are conflict-free); per-element operation order as before.
  for (int k = 0; k < N; ++k) {
    double piv = L.H[2 * N * k + k];
    for (int r = lane; r < N; r += 64) L.fac[r] = L.H[2 * N * r + k];
    __syncthreads();
    for (int c = lane; c < 2 * N; c += 64) dd_hinv_update_col(L.H, 2 * N, N, L.fac, piv, k, c);
    __syncthreads();
  }
  double* out = a.dHinv + (size_t)sc * N * N;
  for (int e = lane; e < N * N; e += 64) out[e] = L.H[2 * N * (e / N) + N + (e % N)];
}

// k_dd_key: drain-order key of every scenario -- the previous step's (DD iteration count, slowest agent
// QP's IPM iterations), longest first, as k_cadmm's key -- sorted by k_bucket into one queue (class 0).
// (dd_ipm_bin: dat_dd_step.hpp)
__global__ void k_dd_key(KArgs a) {
  const int sc = blockIdx.x * blockDim.x + threadIdx.x;
  if (sc < a.B) a.need[sc] = NIB - 1 - (NPB * iter_bin(a.iters[sc]) + dd_ipm_bin(a.ipmx[sc]));
}

}  // namespace

namespace dat {

size_t dd_lds(int n, bool env) { return dd_carve(nullptr, n, env).bytes(); }
size_t dd_setup_lds(int n) { return dd_setup_carve(nullptr, n).bytes(); }

// k_dd_setup<n>: [H | I] in registers to n = DD_REG_NMAX, <0>: in LDS, beyond the default 64 KB of dynamic LDS from
// n = 11 on
hipError_t launch_k_dd_setup(int blocks, size_t lds, hipStream_t st, const KArgs& a) {
  using K = void (*)(KArgs);
  static const K reg[] = {k_dd_setup<3>, k_dd_setup<4>, k_dd_setup<5>, k_dd_setup<6>, k_dd_setup<7>, k_dd_setup<8>};
  static_assert(DD_REG_NMAX == 8, "k_dd_setup<n>: one instantiation per n in [3, DD_REG_NMAX]");
  const int n = a.n;
  if (n > DD_REG_NMAX)
    if (const hipError_t e = hipFuncSetAttribute((const void*)k_dd_setup<0>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        e != hipSuccess)
      return e;
  hipLaunchKernelGGL(n <= DD_REG_NMAX ? reg[n - 3] : k_dd_setup<0>, dim3(blocks), dim3(64), lds, st, a);
  return hipGetLastError();
}
hipError_t launch_k_dd_key(hipStream_t st, const KArgs& a) {
  hipLaunchKernelGGL(k_dd_key, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace dat
