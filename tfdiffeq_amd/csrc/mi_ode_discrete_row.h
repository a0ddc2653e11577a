// The reverse sweep of a fixed-grid solve for a row-local f with a generated vjp (tfdiffeq_amd/lower.py: reverse mode over the trace of
// a Python callable): the whole backward of odeint_discrete, all steps, in ONE launch.
//
//   discrete_row_step     one step of one trajectory, host/device: recomputes the s <= 4 stage states Y_i once, then for i = s .. 1
//                         kbar_i = h b_i lambda_{n+1} + h sum_{j>i} a_ji Ybar_j,  (Ybar_i, theta contributions) = f.vjp(t_n + c_i h, Y_i, kbar_i)
//                         and lambda_n = lambda_{n+1} + sum_i Ybar_i.  No HIP construct: the CPU tests compile it with g++.
//   k_discrete_rowlocal   a trajectory per lane (wave64, 256 threads, workgroups stride over groups of 256 rows).  A lane walks
//                         n = N-2 .. 0 from the stored forward solution.  Every parameter contribution is summed over the 64 lanes by a
//                         fixed-order butterfly and added by lane 0 to the wavefront's own partial [P] in LDS; at the end the wave partials
//                         are folded in wave order into the workgroup's row of a [grid, P] buffer, and the LAST workgroup to arrive (a
//                         ticket taken after the write-through stores have drained) folds the rows in workgroup order.  No
//                         floating-point atomics, no workgroup waits for another: two calls agree in every bit and the grid needs no
//                         co-residency.
#pragma once

#ifndef MI_ODE_ROW_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_ODE_ROW_HD __host__ __device__ __forceinline__
#else
#define MI_ODE_ROW_HD inline
#endif
#endif

namespace mi {

constexpr int kDiscreteRowMaxStages = 4;
constexpr int kDiscreteRowMaxParams = 1024;      // LDS: 4 wavefronts x P x 8 bytes = 32 KB of the CU's 160 KB
constexpr int kDiscreteRowThreads = 256;         // the workgroup of k_fixed_rowlocal
constexpr int kDiscreteRowMaxGrid = 1024;

struct DiscreteRowTableau {
  double a[kDiscreteRowMaxStages][kDiscreteRowMaxStages];   // a[i][j], j < i: the weight of k_j in Y_i
  double b[kDiscreteRowMaxStages];
  double c[kDiscreteRowMaxStages];
};

// One step, one trajectory.  S is a template parameter so that every index into the stage storage is a compile-time constant (a
// runtime-indexed private array lives in scratch memory).  lam_out must not alias lam_in.
template <typename T, int S, int D, class RHS, class ACC>
MI_ODE_ROW_HD void discrete_row_step(const RHS& f, const DiscreteRowTableau& tb, const T* yn, T tn, T h, const T* lam_in, T* lam_out, ACC& acc) {
  T Y[S][D], Yb[S][D], K[S > 1 ? S - 1 : 1][D];
#pragma unroll
  for (int d = 0; d < D; ++d) Y[0][d] = yn[d];
#pragma unroll
  for (int i = 1; i < S; ++i) {
    f(tn + (T)tb.c[i - 1] * h, Y[i - 1], K[i - 1]);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      T s = (T)0;
#pragma unroll
      for (int j = 0; j < i; ++j)
        if (tb.a[i][j] != 0.0) s += (T)tb.a[i][j] * K[j][d];
      Y[i][d] = yn[d] + h * s;
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) lam_out[d] = lam_in[d];
#pragma unroll
  for (int i = S - 1; i >= 0; --i) {
    T kb[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      T s = (T)tb.b[i] * lam_in[d];
#pragma unroll
      for (int j = i + 1; j < S; ++j)
        if (tb.a[j][i] != 0.0) s += (T)tb.a[j][i] * Yb[j][d];
      kb[d] = h * s;
    }
    f.vjp(tn + (T)tb.c[i] * h, Y[i], kb, Yb[i], acc);
#pragma unroll
    for (int d = 0; d < D; ++d) lam_out[d] += Yb[i][d];
  }
}

}  // namespace mi

#if defined(__HIPCC__)
#include "mi_ode_dev.h"

namespace mi {

struct DiscreteRowArgs {
  const void* ys;              // [N, batch, D] the forward solution
  const void* gys;             // [N, batch, D] the gradient of the loss with respect to it
  void* gy0;                   // [batch, D]
  void* gtheta;                // [P]
  void* partials;              // [grid, P] workspace
  unsigned* ticket;            // device word, zero between launches
  const double* t;             // device: the N grid times, float64 (values already rounded to the state dtype)
  long long batch;
  int n_points, n_params, stages;
  DiscreteRowTableau tb;
  RhsParams rhs;
};

// the sink the generated vjp adds its parameter contributions to: sum over the wavefront, lane 0 keeps it
template <typename T>
struct DiscreteRowAcc {
  T* part;                     // this wavefront's [P] in LDS
  bool live;                   // the lane has a trajectory (a lane without one takes part in every butterfly with zeros)
  int lane;
  __device__ __forceinline__ void add(int i, T v) {
    v = live ? v : (T)0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) part[i] += v;
  }
};

__device__ __forceinline__ void dr_store_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dr_store_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float dr_load_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double dr_load_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T, class RHS, int S>
__global__ __launch_bounds__(kDiscreteRowThreads) void k_discrete_rowlocal(DiscreteRowArgs A) {
  constexpr int D = RHS::D;
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
    DiscreteRowAcc<T> acc{s_part + wave * P, live, lane};
    const long long e0 = row * D;
    T lam[D], lam2[D], yn[D];
#pragma unroll
    for (int d = 0; d < D; ++d) lam[d] = live ? gys[(long long)(N - 1) * plane + e0 + d] : (T)0;
    for (int n = N - 2; n >= 0; --n) {
      const T tn = (T)A.t[n];
      const T h = (T)A.t[n + 1] - tn;                        // per step: the grid may be non-uniform or decreasing
#pragma unroll
      for (int d = 0; d < D; ++d) yn[d] = live ? ys[(long long)n * plane + e0 + d] : (T)0;
      discrete_row_step<T, S, D>(rhs, A.tb, yn, tn, h, lam, lam2, acc);
#pragma unroll
      for (int d = 0; d < D; ++d) lam[d] = lam2[d] + (live ? gys[(long long)n * plane + e0 + d] : (T)0);
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

// what a discrete plugin (csrc/mi_ode_discrete_plugin.h) instantiates for its functor
template <typename T, class RHS>
struct DiscreteRowLaunch {
  static int sweep(const DiscreteRowArgs* A, int grid, hipStream_t st) {
    const void* fn = A->stages == 1 ? (const void*)k_discrete_rowlocal<T, RHS, 1>
                   : A->stages == 2 ? (const void*)k_discrete_rowlocal<T, RHS, 2>
                   : A->stages == 4 ? (const void*)k_discrete_rowlocal<T, RHS, 4> : nullptr;
    if (fn == nullptr || grid < 1 || grid > kDiscreteRowMaxGrid || A->n_params != RHS::P || A->n_params > kDiscreteRowMaxParams) return MI_ODE_E_INVALID;
    const size_t lds = (size_t)(kDiscreteRowThreads / 64) * (size_t)(A->n_params > 0 ? A->n_params : 1) * sizeof(T);
    void* args[] = {(void*)A};
    if (hipLaunchKernel(fn, dim3((unsigned)grid), dim3(kDiscreteRowThreads), args, lds, st) != hipSuccess) return MI_ODE_E_HIP;
    return 0;
  }
};

}  // namespace mi

#define MI_ODE_DISCRETE_PLUGIN_ABI 0x44520001
struct mi_ode_discrete_row_plugin {
  int abi;                       // MI_ODE_DISCRETE_PLUGIN_ABI (also tells it apart from the other tables that travel in mi_ode_rhs.plugin)
  int dtype;                     // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int n_params;                  // P: the range of the vjp's acc.add index
  int (*launch_sweep)(const mi::DiscreteRowArgs* A, int grid, hipStream_t st);
};
#endif  // __HIPCC__
