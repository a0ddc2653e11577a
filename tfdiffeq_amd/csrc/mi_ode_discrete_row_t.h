// The reverse sweep of a fixed-grid solve with PER-ROW times and lengths (csrc/mi_ode_fixed_rows_t.h) for a row-local f with a generated
// vjp: the whole backward of odeint_discrete with a 2-D `t`, all rows and all steps, in ONE launch.
//
// k_discrete_rowlocal_t is k_discrete_rowlocal (mi_ode_discrete_row.h) with a per-lane view: every lane reads its own row of t [batch][T]
// and its own length, and calls the UNCHANGED discrete_row_step.  The parameter sink (DiscreteRowAcc::add) is a 64-lane butterfly, so
// every lane of a wavefront makes the same number of discrete_row_step calls: the step loop runs over a wave-uniform range, down from
// the wavefront's largest length, and a lane is ACTIVE in step n only when it has a row and n <= len - 2.  An inactive lane runs the step
// with yn = 0 and h = 0 - every kbar is then h * (..) = 0 - its contributions are masked to exactly 0, as those of lanes without a
// trajectory already are, and what the step returns for it is dropped: its own lam is not disturbed.  (It is handed its own lam, not a
// zeroed copy: the copy and its selects cost 84 spilled registers in the float64 rk4 instantiation of an 8-element functor.)  A row picks up lam = gys[len - 1] when its own last step comes up, then lam = lam2 + gys[n] per step; len == 1 gives
// gy0 = gys[0] and no parameter contribution.  gys[k][row] for k >= len and t[row][len ..] are never read.  Times are read as given
// (h is negative for a decreasing row, sign 1).
// The rest is k_discrete_rowlocal's: the LDS partials per wavefront, the [grid, P] rows, the ticket after drained write-through stores,
// the last workgroup folding in workgroup order - no floating-point atomics, no workgroup waits for another, the ticket zero at exit.
#pragma once
#include "mi_ode_discrete_row.h"

#if defined(__HIPCC__)
namespace mi {

struct DiscreteRowTArgs {
  DiscreteRowArgs r;           // as k_discrete_rowlocal gets them; r.n_points = T (the longest row); r.t is not read
  const double* t;             // device [batch][T]: row i's times are t[i][0 .. len[i] - 1] (values already rounded to the state dtype)
  const int* len;              // device [batch], values 1 .. T; null: every row has T times
};

template <typename T, class RHS, int S>
__global__ __launch_bounds__(kDiscreteRowThreads) void k_discrete_rowlocal_t(DiscreteRowTArgs R) {
  constexpr int D = RHS::D;
  const DiscreteRowArgs& A = R.r;
  extern __shared__ double dr_smem_[];
  T* s_part = (T*)dr_smem_;                                  // [4 wavefronts][P]
  __shared__ int s_last;
  const int P = A.n_params, N = A.n_points;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  constexpr int kWaves = kDiscreteRowThreads / 64;
  for (int i = (int)threadIdx.x; i < kWaves * P; i += kDiscreteRowThreads) s_part[i] = (T)0;
  __syncthreads();
  const RHS rhs(A.rhs);
  const T* ys = (const T*)A.ys;
  const T* gys = (const T*)A.gys;
  T* gy0 = (T*)A.gy0;
  const long long plane = A.batch * D;                       // elements of one grid point
  const long long groups = (A.batch + kDiscreteRowThreads - 1) / kDiscreteRowThreads;
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long long row = g * kDiscreteRowThreads + threadIdx.x;
    const bool live = row < A.batch;                         // no lane leaves: the butterflies need all 64
    // the lane's own view of the call
    const double* t_row = R.t + (live ? row : 0) * N;
    int len = 1;
    if (live) {
      len = R.len != nullptr ? R.len[row] : N;
      len = len < 1 ? 1 : (len > N ? N : len);               // (the host refuses such a length; no read outside the row either way)
    }
    DiscreteRowAcc<T> acc{s_part + wave * P, false, lane};
    const long long e0 = row * D;
    T lam[D], lam2[D], yn[D];
#pragma unroll
    for (int d = 0; d < D; ++d) lam[d] = live ? gys[(long long)(len - 1) * plane + e0 + d] : (T)0;
    int wlen = len;                                          // the wavefront's longest row: the same value in all 64 lanes
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(wlen, m, 64); wlen = o > wlen ? o : wlen; }
    for (int n = wlen - 2; n >= 0; --n) {                    // wave-uniform: every lane makes the same wlen - 1 calls
      const bool active = live && n <= len - 2;
      acc.live = active;
      const T tn = active ? (T)t_row[n] : (T)0;
      const T h = active ? (T)t_row[n + 1] - tn : (T)0;      // per step: the row's grid may be non-uniform or decreasing
#pragma unroll
      for (int d = 0; d < D; ++d) yn[d] = active ? ys[(long long)n * plane + e0 + d] : (T)0;
      discrete_row_step<T, S, D>(rhs, A.tb, yn, tn, h, lam, lam2, acc);
      if (active) {
#pragma unroll
        for (int d = 0; d < D; ++d) lam[d] = lam2[d] + gys[(long long)n * plane + e0 + d];
      }
    }
    if (live) {
#pragma unroll
      for (int d = 0; d < D; ++d) gy0[e0 + d] = lam[d];
    }
  }
  __syncthreads();
  // wave partials, in wave order, into this workgroup's row (write-through stores: the last workgroup reads them past its L1)
  T* mine = (T*)A.partials + (long long)blockIdx.x * P;
  for (int i = (int)threadIdx.x; i < P; i += kDiscreteRowThreads) {
    T s = s_part[i];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += s_part[w * P + i];
    dr_store_agent(mine + i, s);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this thread's stores have landed before the workgroup's ticket says so
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned tk = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (tk == gridDim.x - 1);
  }
  __syncthreads();
  if (!s_last) return;
  const T* all = (const T*)A.partials;
  T* out = (T*)A.gtheta;
  for (int i = (int)threadIdx.x; i < P; i += kDiscreteRowThreads) {
    T s = (T)0;
    for (unsigned b = 0; b < gridDim.x; ++b) s += dr_load_agent(all + (long long)b * P + i);   // workgroup order
    out[i] = s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a discrete-t plugin (csrc/mi_ode_discrete_t_plugin.h) instantiates for its functor
template <typename T, class RHS>
struct DiscreteRowTLaunch {
  static int sweep(const DiscreteRowTArgs* R, int grid, hipStream_t st) {
    const DiscreteRowArgs* A = &R->r;
    const void* fn = A->stages == 1 ? (const void*)k_discrete_rowlocal_t<T, RHS, 1>
                   : A->stages == 4 ? (const void*)k_discrete_rowlocal_t<T, RHS, 4> : nullptr;
    if (fn == nullptr || grid < 1 || grid > kDiscreteRowMaxGrid || A->n_params != RHS::P || A->n_params > kDiscreteRowMaxParams) return MI_ODE_E_INVALID;
    const size_t lds = (size_t)(kDiscreteRowThreads / 64) * (size_t)(A->n_params > 0 ? A->n_params : 1) * sizeof(T);
    void* args[] = {(void*)R};
    if (hipLaunchKernel(fn, dim3((unsigned)grid), dim3(kDiscreteRowThreads), args, lds, st) != hipSuccess) return MI_ODE_E_HIP;
    return 0;
  }
};

}  // namespace mi

#define MI_ODE_DISCRETE_T_PLUGIN_ABI 0x44540001
struct mi_ode_discrete_row_t_plugin {
  int abi;                       // MI_ODE_DISCRETE_T_PLUGIN_ABI (also tells it apart from the other tables that travel in mi_ode_rhs.plugin)
  int dtype;                     // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int n_params;                  // P: the range of the vjp's acc.add index
  int (*launch_sweep)(const mi::DiscreteRowTArgs* R, int grid, hipStream_t st);
};
#endif  // __HIPCC__
