// Per-trajectory step control with PER-ROW output times, lengths and tolerances: a 2-D `t`, options['t_lengths'], rtol / atol of shape
// [batch] under options={'per_trajectory': True} / mi_ode_integrate_rows_t.
//
// k_rows_rowlocal (mi_ode_rows.h) hands every lane the same view of the call: one t_start, one array of output times, one n_out, one
// CtrlParams.  rows_integrate (mi_ode_rows_core.h) never needed that: it takes them per call.  Here every lane builds its own view
//   t_start = t[row][0],  cp.t_out = &t[row][1],  n_out = len[row] - 1,  cp.rtol = rtol[row],  cp.atol = atol[row]
// and calls the UNCHANGED rows_integrate: row i is what the shared kernel returns for (y0[i:i+1], t[i, :len_i]) at the row's own
// tolerances, bit for bit, as in mi_ode_rows.h.
//   * the geometry of k_rows_rowlocal: one trajectory per thread, 256-thread workgroups, grid = ceil(batch / 256), no hand-off between
//     workgroups, no barrier at all (nothing is staged: a lane reads its times through its own pointer into global memory - the handful
//     of loads per accepted step that attempt_core's output cursor and step_emit make sit behind S right-hand-side evaluations);
//   * a lane's loop ends by attempt_tail alone, as there.  The output cursor is bounded by n_out <= T - 1 (the kernel clamps len[row]
//     to 1 .. T itself), so whatever the times hold - unordered values, NaN - a lane reads inside its row of t, writes inside its row
//     of the solution and stops: with wrong numbers or a status bit, never with an unbounded loop;
//   * solution[k, row] for k >= len[row] is written as exact zeros by the lane after its loop; t[row, len[row]:] is never read;
//   * [batch, 4] row results and the per-wavefront summary as k_rows_rowlocal leaves them.
#pragma once
#include "mi_ode_rows.h"

#define MI_ODE_ROWS_T_PLUGIN_ABI 1

// what a rows-t plugin exports (mi_ode_rows_t_plugin.h): the k_rows_rowlocal_t instantiations of a user's functor
struct mi_ode_rows_t_plugin {
  int abi;                     // MI_ODE_ROWS_T_PLUGIN_ABI
  int dtype;                   // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int reserved;
  const void* (*rows_t_fn)(int S, int ts_dense, int fsal);    // k_rows_rowlocal_t instantiation, or null
};

namespace mi {

struct RowsTArgs {
  RowsArgs r;                  // as k_rows_rowlocal gets them; p.n_out = T - 1 (the longest row); p.t0 / p.t_small / p.s.t_out are not read
  const double* t;             // device [batch][T]: row i's times are t[i][0 .. len[i] - 1], strictly increasing
  const int* len;              // device [batch], values 1 .. T; null: every row has T times
  const double* rtol;          // device [batch]; null: the handle's rtol for every row
  const double* atol;          // device [batch]; null: the handle's atol
  int T;
};

template <typename T, int S, bool TS, class RHS, bool FSAL = true>
__global__ __launch_bounds__(256) void k_rows_rowlocal_t(RowsTArgs R) {
  static_assert(!rhs_is_coop<RHS>::value, "a cooperative right-hand side has barriers inside f: never under per-lane control flow");
  constexpr int D = RHS::D;
  using Row = RowVec<T, D>;
  const PersistArgs& A = R.r.p;
  const RHS rhs(A.s.rhs);
  const T sign = (T)A.s.rhs.sign;
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = row < A.s.batch;
  const long long e0 = row * D;

  RowResult res;
  res.n_attempt = res.n_accept = res.nfe = 0; res.status = 0;
  if (live) {
    // the lane's own view of the call
    const double* tr = R.t + row * R.T;
    int len = R.len != nullptr ? R.len[row] : R.T;
    len = len < 1 ? 1 : (len > R.T ? R.T : len);               // (the host refuses such a length; no read or write outside the row either way)
    CtrlParams cp = A.s.cp;
    cp.t_out = tr + 1;
    if (R.rtol != nullptr) cp.rtol = R.rtol[row];
    if (R.atol != nullptr) cp.atol = R.atol[row];
    T y[D], f[D];
    {
      const Row y0 = *(const Row*)((const T*)A.y0 + e0);
      *(Row*)((T*)A.out0 + e0) = y0;                          // solution[0] = y0 (solvers.py:30)
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = y0.v[d];
    }
    rows_integrate<T, S, TS, FSAL, RHS>(rhs, A.s, cp, sign, tr[0], A.first_dt, len - 1, y, f, e0, res);
    // the padding of a short row: exact zeros (solution[k] = out0 + k planes)
    {
      Row z;
#pragma unroll
      for (int d = 0; d < D; ++d) z.v[d] = (T)0;
      for (int k = len; k < R.T; ++k) *(Row*)((T*)A.out0 + (long long)k * A.s.n_plane + e0) = z;
    }
    // the final state: planes 0 / 2, where k_persist_rowlocal leaves y and f (mi_ode_get_state)
    Row yo, fo;
#pragma unroll
    for (int d = 0; d < D; ++d) { yo.v[d] = y[d]; fo.v[d] = f[d]; }
    *(Row*)((T*)A.s.planes + e0) = yo;
    *(Row*)((T*)(A.s.planes + 2 * A.s.stride) + e0) = fo;
    long long* o = R.r.row_stats + row * 4;
    o[0] = res.n_attempt; o[1] = res.n_accept; o[2] = res.nfe; o[3] = (long long)res.status;
  }
  // every lane is back: the call's summary, one set of atomics per wavefront
  const long long m_att = rows_wave_max(res.n_attempt), m_acc = rows_wave_max(res.n_accept);
  const long long m_rej = rows_wave_max(res.n_attempt - res.n_accept), m_nfe = rows_wave_max(res.nfe);
  unsigned bits = res.status;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bits |= (unsigned)__shfl_down((int)bits, off, 64);
  if ((threadIdx.x & 63) == 0) {
    __hip_atomic_fetch_max(&R.r.agg->n_attempt, m_att, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&R.r.agg->n_accept, m_acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&R.r.agg->n_reject, m_rej, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&R.r.agg->nfe, m_nfe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bits != 0u) __hip_atomic_fetch_or(&R.r.agg->status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {                  // (fields no atomic above touches)
    Ctl* g = R.r.agg;
    g->idx_y0 = 0; g->idx_y1 = 1;
    for (int j = 0; j < kMaxK; ++j) g->idx_k[j] = 2 + j;
    g->t0 = g->t1 = 0.0;                                      // (every row ends at a time of its own: the call has no single one)
    g->done = 1;
  }
}

// the instantiation set of RowsKernels::fn
template <typename T, class RHS>
struct RowsTKernels {
  static const void* fn(int S, int ts_dense, int fsal) {
    if (S == 6 && fsal) return ts_dense ? (const void*)k_rows_rowlocal_t<T, 6, true, RHS> : (const void*)k_rows_rowlocal_t<T, 6, false, RHS>;
    if (S == 3 && fsal && !ts_dense) return (const void*)k_rows_rowlocal_t<T, 3, false, RHS>;
    if (S == 13 && fsal && !ts_dense) return (const void*)k_rows_rowlocal_t<T, 13, false, RHS, true>;
    if (S == 1 && !fsal && !ts_dense) return (const void*)k_rows_rowlocal_t<T, 1, false, RHS, false>;
    return nullptr;
  }
};

}  // namespace mi

// the catalogue families' kernels, one translation unit per state dtype (mi_ode_rows_t.hip, mi_ode_rows_t_f32.hip)
const void* mi_rows_t_fn_f64(int family, int S, int ts_dense, int fsal);
const void* mi_rows_t_fn_f32(int family, int S, int ts_dense, int fsal);
