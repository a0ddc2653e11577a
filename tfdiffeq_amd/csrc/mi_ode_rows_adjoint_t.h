// Gradients for per-trajectory solves with PER-ROW output times, lengths and tolerances: the whole backward of
// odeint_adjoint(..., t [batch, T], options={'per_trajectory': True, 't_lengths': ..}) in ONE launch / mi_ode_adjoint_rows_t.
//
// k_rows_adjoint (mi_ode_rows_adjoint.h) hands every lane the same output times, one n_t and one CtrlParams.  rows_adjoint_row
// (mi_ode_rows_adjoint_core.h) never needed that: it takes them per call.  Here every lane builds its own view
//   neg_t = &neg_t[row][0],  n_t = len[row],  cp.rtol = rtol[row],  cp.atol = atol[row]
// and calls the UNCHANGED rows_adjoint_row: row i is what k_rows_adjoint returns for (ans[:len_i, i:i+1], g[:len_i, i:i+1], t[i, :len_i])
// at the row's own tolerances, bit for bit.
//   * the geometry of k_rows_adjoint: one trajectory per thread, 256-thread workgroups, grid = ceil(batch / 256), no grid hand-off.
//     Nothing is staged: a lane reads its times through its own pointer into global memory, so no barrier precedes the lanes' loops;
//   * a lane's loops end by attempt_tail alone, as there; the interval loop is bounded by len[row] <= T (the kernel clamps it to 1 .. T
//     itself), so whatever the times hold a lane reads inside its row of neg_t, ans and g and writes inside its rows of the outputs;
//   * neg_t[row][len ..] and g[k][row] for k >= len are never read; time_vjps[row][k] for k >= len and the counts of the intervals
//     beyond the row's length are exact zeros.  rows_adjoint_row packs a row's counts as [3][len - 1]; the lane spreads them to the
//     [3][T - 1] of its row afterwards, in place, from the back;
//   * the time gradient is the rows' own (row_time_vjps [batch, T]) and is NOT summed.  Only adj_params is folded: the workgroup's rows
//     in row order into its row of a [grid, max(P, 1)] buffer, the workgroups in order by the last one to arrive - k_rows_adjoint's
//     ticket after drained write-through stores: no floating-point atomics, two calls agree in every bit.
#pragma once
#include "mi_ode_rows_adjoint.h"

#define MI_ODE_ROWS_ADJOINT_T_PLUGIN_ABI 0x41540001

namespace mi {

struct RowsAdjTArgs {
  RowsAdjArgs a;               // as k_rows_adjoint gets them, but: neg_t is [batch][T], n_t = T (the longest row), partials is
                               // [grid, max(P, 1)] and grad_t is not written (null)
  const int* len;              // device [batch], values 1 .. T; null: every row has T times
  const double* rtol;          // device [batch]; null: the descriptor's rtol for every row
  const double* atol;          // device [batch]; null: the descriptor's atol
};

template <typename T, int S, class RHS>
__global__ __launch_bounds__(kRowsAdjThreads) void k_rows_adjoint_t(RowsAdjTArgs R) {
  static_assert(!rhs_is_coop<RHS>::value, "a cooperative right-hand side has barriers inside f: never under per-lane control flow");
  using L = AdjLayout<RHS>;
  static_assert(L::NA <= kRowsAdjMaxAug, "the augmented state of a row is thread-private: 2 D + 1 + P <= 32");
  constexpr int D = L::D, PP = L::PP;
  __shared__ int s_last;
  const RowsAdjArgs& A = R.a;
  const int n_t = A.n_t;
  const RHS rhs(A.s.rhs);
  const long long row = (long long)blockIdx.x * kRowsAdjThreads + threadIdx.x;
  const long long plane = A.batch * D;
  T* row_params = (T*)A.row_params;
  if (row < A.batch) {
    // the lane's own view of the call
    int len = R.len != nullptr ? R.len[row] : n_t;
    len = len < 1 ? 1 : (len > n_t ? n_t : len);               // (the host refuses such a length; no read or write outside the row either way)
    CtrlParams cp = A.s.cp;
    if (R.rtol != nullptr) cp.rtol = R.rtol[row];
    if (R.atol != nullptr) cp.atol = R.atol[row];
    AdjRowIO<T> io;
    io.ans = (const T*)A.ans + row * D;
    io.g = (const T*)A.g + row * D;
    io.plane = plane;
    io.grad_y0 = (T*)A.grad_y0 + row * D;
    io.grad_params = row_params + row * PP;
    io.time_vjps = (T*)A.row_tvjp + row * n_t;
    io.counts = A.row_counts + row * 3 * (n_t - 1);
    const unsigned status = rows_adjoint_row<T, S, RHS>(rhs, A.s, cp, A.neg_t + row * n_t, len, io);
    A.row_status[row] = (long long)status;
    // the padding of a short row: exact zeros.  Counts: [3][len - 1] packed -> [3][n_t - 1]; a target index is never below its source
    // and the walk is from the back, so no source is overwritten before it is read
    for (int k = len; k < n_t; ++k) io.time_vjps[k] = (T)0;
    if (len < n_t) {
      for (int c = 2; c >= 0; --c)
        for (int i = n_t - 2; i >= 0; --i) {
          const long long v = i < len - 1 ? io.counts[c * (len - 1) + i] : 0;
          io.counts[c * (n_t - 1) + i] = v;
        }
    }
  }
  // every lane is back.  The workgroup's adj_params, in row order, into its row of the [grid, PP] buffer (write-through: the last
  // workgroup reads them past its L1)
  __syncthreads();
  const long long first = (long long)blockIdx.x * kRowsAdjThreads;
  const int live = (int)((A.batch - first) < kRowsAdjThreads ? (A.batch - first) : kRowsAdjThreads);
  T* mine = (T*)A.partials + (long long)blockIdx.x * PP;
  for (int j = (int)threadIdx.x; j < PP; j += kRowsAdjThreads) {
    T s = (T)0;
    for (int r = 0; r < live; ++r) s += row_params[(first + r) * PP + j];
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
  for (int j = (int)threadIdx.x; j < PP; j += kRowsAdjThreads) {
    T s = (T)0;
    for (unsigned b = 0; b < gridDim.x; ++b) s += ra_load_agent(all + (long long)b * PP + j);   // workgroup order
    ((T*)A.grad_params)[j] = s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a rows-adjoint-t plugin (csrc/mi_ode_rows_adjoint_t_plugin.h) instantiates for its functor: the set of RowsAdjLaunch
template <typename T, class RHS>
struct RowsAdjTLaunch {
  static int launch(const RowsAdjTArgs* R, int S, int grid, hipStream_t st) {
    const void* fn = S == 6 ? (const void*)k_rows_adjoint_t<T, 6, RHS> : S == 3 ? (const void*)k_rows_adjoint_t<T, 3, RHS> : nullptr;
    if (fn == nullptr || grid < 1 || (long long)grid * kRowsAdjThreads < R->a.batch) return MI_ODE_E_INVALID;
    void* args[] = {(void*)R};
    if (hipLaunchKernel(fn, dim3((unsigned)grid), dim3(kRowsAdjThreads), args, 0, st) != hipSuccess) return MI_ODE_E_HIP;
    return 0;
  }
};

}  // namespace mi

struct mi_ode_rows_adjoint_t_plugin {
  int abi;                       // MI_ODE_ROWS_ADJOINT_T_PLUGIN_ABI (also tells it apart from the other tables that travel in mi_ode_rhs.plugin)
  int dtype;                     // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int n_params;                  // P: the range of the vjp's acc.add index
  int (*launch)(const mi::RowsAdjTArgs* R, int S, int grid, hipStream_t st);
};
