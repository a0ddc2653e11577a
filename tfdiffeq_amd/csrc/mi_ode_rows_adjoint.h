// Gradients for per-trajectory solves: the whole backward of odeint_adjoint(..., options={'per_trajectory': True}) in ONE launch.
//
// k_rows_adjoint: every lane is the reference's adjoint algorithm for ITS trajectory (rows_adjoint_row, mi_ode_rows_adjoint_core.h): all
// T - 1 intervals, each an adaptive integration of the row's own augmented tuple state with the reference's per-component control.
//   * one trajectory per thread, 256-thread workgroups, grid = ceil(batch / 256) for any batch size;
//   * the (negated) output times are staged in LDS once, before any lane's loop; the barrier after it is the only one that precedes the
//     per-lane control flow.  Workgroups never wait for each other: no grid hand-off, no co-residency;
//   * a lane's loops end by attempt_tail alone (outputs produced, max_num_steps, t + dt == t); a row that fails keeps ITS status and
//     stops, the others carry on.  Dead lanes of the last workgroup never enter rows_adjoint_row;
//   * cooperative right-hand sides can never be instantiated here (a barrier under divergent control flow hangs);
//   * every row writes its own adj_params [P] and time vjps [T]: nothing is reduced inside the loops.  After the lanes are back the
//     workgroup folds its rows in row order into its row of a [grid, P + T] buffer (write-through stores), and the LAST workgroup to
//     arrive - a ticket taken after those stores have drained, the pattern of mi_ode_discrete_row.h - folds the workgroups in order:
//     no floating-point atomics, nobody waits, two calls agree in every bit.
// Registers: the stage derivatives k[S + 1][NA] of the augmented state (NA = 2 D + 1 + P <= 32) are thread-private and indexed by
// constants only; what does not fit the 512 registers a lane of a 256-thread workgroup can have goes to scratch (docs/KERNELS.md lists
// every instantiation's resource report).
#pragma once
#include "mi_ode_persist.h"
#include "mi_ode_rows_core.h"
#include "mi_ode_rows_adjoint_core.h"

#define MI_ODE_ROWS_ADJOINT_PLUGIN_ABI 0x41520001

namespace mi {

constexpr int kRowsAdjThreads = 256;
constexpr int kRowsAdjTimes = 256;               // output times staged in LDS (more: read from the device array)
constexpr int kRowsAdjMaxAug = 32;               // NA = 2 D + 1 + max(P, 1): the row-local limit of the forward kernels

struct RowsAdjArgs {
  StepArgs s;                  // tableau, right-hand side parameters, controller parameters (planes / ctl / out unused)
  const void* ans;             // [T, batch, D] the forward solution
  const void* g;               // [T, batch, D] the gradient of the loss with respect to it
  void* grad_y0;               // [batch, D]
  void* row_params;            // [batch, max(P, 1)]
  void* row_tvjp;              // [batch, T]
  long long* row_counts;       // [batch, 3, T - 1]: attempts, accepted steps, function evaluations per interval
  long long* row_status;       // [batch]
  void* grad_params;           // [max(P, 1)]: the rows summed in a fixed order
  void* grad_t;                // [T]
  void* partials;              // [grid, max(P, 1) + T] workspace
  unsigned* ticket;            // device word, zero between launches
  const double* neg_t;         // device [T]: the output times, negated (the backward solves run in the solver's time s = -t)
  long long batch;
  int n_t;
};

__device__ __forceinline__ void ra_store_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ra_store_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ra_load_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ra_load_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T, int S, class RHS>
__global__ __launch_bounds__(kRowsAdjThreads) void k_rows_adjoint(RowsAdjArgs A) {
  static_assert(!rhs_is_coop<RHS>::value, "a cooperative right-hand side has barriers inside f: never under per-lane control flow");
  using L = AdjLayout<RHS>;
  static_assert(L::NA <= kRowsAdjMaxAug, "the augmented state of a row is thread-private: 2 D + 1 + P <= 32");
  constexpr int D = L::D, PP = L::PP;
  __shared__ double s_nt[kRowsAdjTimes];
  __shared__ int s_last;
  const int n_t = A.n_t;
  const double* neg_t = A.neg_t;
  if (n_t <= kRowsAdjTimes) {
    for (int i = (int)threadIdx.x; i < n_t; i += kRowsAdjThreads) s_nt[i] = A.neg_t[i];
    neg_t = s_nt;
  }
  __syncthreads();                                           // before any lane's loop
  const RHS rhs(A.s.rhs);
  const long long row = (long long)blockIdx.x * kRowsAdjThreads + threadIdx.x;
  const long long plane = A.batch * D;
  T* row_params = (T*)A.row_params;
  T* row_tvjp = (T*)A.row_tvjp;
  if (row < A.batch) {
    AdjRowIO<T> io;
    io.ans = (const T*)A.ans + row * D;
    io.g = (const T*)A.g + row * D;
    io.plane = plane;
    io.grad_y0 = (T*)A.grad_y0 + row * D;
    io.grad_params = row_params + row * PP;
    io.time_vjps = row_tvjp + row * n_t;
    io.counts = A.row_counts + row * 3 * (n_t - 1);
    const unsigned status = rows_adjoint_row<T, S, RHS>(rhs, A.s, A.s.cp, neg_t, n_t, io);
    A.row_status[row] = (long long)status;
  }
  // every lane is back.  The workgroup's rows, in row order, into its row of the [grid, W] buffer (write-through: the last workgroup
  // reads them past its L1)
  __syncthreads();
  const int W = PP + n_t;
  const long long first = (long long)blockIdx.x * kRowsAdjThreads;
  const int live = (int)((A.batch - first) < kRowsAdjThreads ? (A.batch - first) : kRowsAdjThreads);
  T* mine = (T*)A.partials + (long long)blockIdx.x * W;
  for (int j = (int)threadIdx.x; j < W; j += kRowsAdjThreads) {
    T s = (T)0;
    if (j < PP) {
      for (int r = 0; r < live; ++r) s += row_params[(first + r) * PP + j];
    } else {
      for (int r = 0; r < live; ++r) s += row_tvjp[(first + r) * n_t + (j - PP)];
    }
    ra_store_agent(mine + j, s);
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
  for (int j = (int)threadIdx.x; j < W; j += kRowsAdjThreads) {
    T s = (T)0;
    for (unsigned b = 0; b < gridDim.x; ++b) s += ra_load_agent(all + (long long)b * W + j);   // workgroup order
    if (j < PP) ((T*)A.grad_params)[j] = s;
    else ((T*)A.grad_t)[j - PP] = s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a rows-adjoint plugin (csrc/mi_ode_rows_adjoint_plugin.h) instantiates for its functor: the two FSAL shaped tableaus with the
// quartic dense output, dopri5 (6 rows) and bosh3 (3 rows)
template <typename T, class RHS>
struct RowsAdjLaunch {
  static int launch(const RowsAdjArgs* A, int S, int grid, hipStream_t st) {
    const void* fn = S == 6 ? (const void*)k_rows_adjoint<T, 6, RHS> : S == 3 ? (const void*)k_rows_adjoint<T, 3, RHS> : nullptr;
    if (fn == nullptr || grid < 1 || (long long)grid * kRowsAdjThreads < A->batch) return MI_ODE_E_INVALID;
    void* args[] = {(void*)A};
    if (hipLaunchKernel(fn, dim3((unsigned)grid), dim3(kRowsAdjThreads), args, 0, st) != hipSuccess) return MI_ODE_E_HIP;
    return 0;
  }
};

}  // namespace mi

struct mi_ode_rows_adjoint_plugin {
  int abi;                       // MI_ODE_ROWS_ADJOINT_PLUGIN_ABI (also tells it apart from the other tables that travel in mi_ode_rhs.plugin)
  int dtype;                     // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int n_params;                  // P: the range of the vjp's acc.add index
  int (*launch)(const mi::RowsAdjArgs* A, int S, int grid, hipStream_t st);
};
