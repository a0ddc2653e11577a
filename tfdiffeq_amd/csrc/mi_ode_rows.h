// Per-trajectory step control for batches of INDEPENDENT row-local systems: options={'per_trajectory': True} / mi_ode_integrate_rows.
//
// The whole-call kernels of mi_ode_persist.h treat a batch as one system, as the reference does: one error norm over all rows, one
// accept decision, one step size, a grid-wide hand-off per attempt.  Here every lane is "thread 0" of its own integration: row i of the
// result is what the shared kernel returns for y0[i:i+1] alone, bit for bit (rows_integrate, mi_ode_rows_core.h, calls the same device
// functions in the same order with the row's own record).
//   * one trajectory per thread, 256-thread workgroups, grid = ceil(batch / 256) for ANY batch size;
//   * workgroups never communicate: no grid hand-off, no co-residency, no planes variant, no spin limits;
//   * the output times are staged in LDS once, before the loop (rows_stage_tout, as persist_stage_tout does); the only barrier of the kernel follows it.  The
//     loop is `while (!st.done)` per lane - a wavefront runs until its slowest lane ends, lanes that are done are masked out by the
//     loop's own control flow, dead lanes of the last workgroup never enter rows_integrate (they evaluate nothing);
//   * a lane's loop ends by attempt_tail alone: all outputs produced, max_num_steps attempts inside one output interval, or
//     t + dt == t.  A row that fails sets ITS status and stops; the other lanes carry on;
//   * cooperative right-hand sides (barriers inside f) can never be instantiated here: a barrier under divergent control flow hangs.
// HBM traffic: y0 in, solution rows out, [batch, 4] int64 of per-row results {attempts, accepted, nfe, status}, the final y / f planes.
#pragma once
#include "mi_ode_persist.h"
#include "mi_ode_rows_core.h"

#define MI_ODE_ROWS_PLUGIN_ABI 1

// what a rows plugin exports (mi_ode_rows_plugin.h): the k_rows_rowlocal instantiations of a user's functor
struct mi_ode_rows_plugin {
  int abi;                     // MI_ODE_ROWS_PLUGIN_ABI
  int dtype;                   // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int reserved;
  const void* (*rows_fn)(int S, int ts_dense, int fsal);      // k_rows_rowlocal instantiation, or null
};

namespace mi {

struct RowsArgs {
  PersistArgs p;               // as the shared whole-call kernel gets them (the hand-off fields are unused)
  long long* row_stats;        // device [batch][4]: attempts, accepted steps, function evaluations, status bits
  Ctl* agg;                    // device, zeroed before the launch: status = OR over rows, n_attempt / n_accept / n_reject / nfe = max over
                               // rows (the maximum is what bounds the time); plane indices as k_persist_rowlocal leaves them
};

// every thread: output times into LDS when they fit, as persist_stage_tout does - with the few that travel as kernel arguments read
// at constant indices (an argument array indexed by the thread number makes the compiler keep a private copy of ALL arguments)
__device__ __forceinline__ const double* rows_stage_tout(const PersistArgs& A, double* lds_tout) {
  if (A.n_out <= kPersistTSmall) {
#pragma unroll
    for (int i = 0; i < kPersistTSmall; ++i)
      if ((int)threadIdx.x == i && i < A.n_out) lds_tout[i] = A.t_small[i];
    return lds_tout;
  }
  if (A.n_out <= kPersistTout) {
    for (int i = threadIdx.x; i < A.n_out; i += blockDim.x) lds_tout[i] = A.s.t_out[i];
    return lds_tout;
  }
  return A.s.t_out;
}

__device__ __forceinline__ long long rows_wave_max(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_down(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

template <typename T, int S, bool TS, class RHS, bool FSAL = true>
__global__ __launch_bounds__(256) void k_rows_rowlocal(RowsArgs R) {
  static_assert(!rhs_is_coop<RHS>::value, "a cooperative right-hand side has barriers inside f: never under per-lane control flow");
  constexpr int D = RHS::D;
  using Row = RowVec<T, D>;
  __shared__ double s_tout[kPersistTout];
  const PersistArgs& A = R.p;
  const RHS rhs(A.s.rhs);
  const T sign = (T)A.s.rhs.sign;
  CtrlParams cp = A.s.cp;
  cp.t_out = rows_stage_tout(A, s_tout);
  __syncthreads();                                            // the one barrier: before any lane's loop
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = row < A.s.batch;
  const long long e0 = row * D;

  RowResult res;
  res.n_attempt = res.n_accept = res.nfe = 0; res.status = 0;
  if (live) {
    T y[D], f[D];
    {
      const Row y0 = *(const Row*)((const T*)A.y0 + e0);
      *(Row*)((T*)A.out0 + e0) = y0;                          // solution[0] = y0 (solvers.py:30)
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = y0.v[d];
    }
    rows_integrate<T, S, TS, FSAL, RHS>(rhs, A.s, cp, sign, A.t0, A.first_dt, A.n_out, y, f, e0, res);
    // the final state: planes 0 / 2, where k_persist_rowlocal leaves y and f (mi_ode_get_state)
    Row yo, fo;
#pragma unroll
    for (int d = 0; d < D; ++d) { yo.v[d] = y[d]; fo.v[d] = f[d]; }
    *(Row*)((T*)A.s.planes + e0) = yo;
    *(Row*)((T*)(A.s.planes + 2 * A.s.stride) + e0) = fo;
    long long* o = R.row_stats + row * 4;
    o[0] = res.n_attempt; o[1] = res.n_accept; o[2] = res.nfe; o[3] = (long long)res.status;
  }
  // every lane is back: the call's summary, one set of atomics per wavefront
  const long long m_att = rows_wave_max(res.n_attempt), m_acc = rows_wave_max(res.n_accept);
  const long long m_rej = rows_wave_max(res.n_attempt - res.n_accept), m_nfe = rows_wave_max(res.nfe);
  unsigned bits = res.status;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bits |= (unsigned)__shfl_down((int)bits, off, 64);
  if ((threadIdx.x & 63) == 0) {
    __hip_atomic_fetch_max(&R.agg->n_attempt, m_att, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&R.agg->n_accept, m_acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&R.agg->n_reject, m_rej, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&R.agg->nfe, m_nfe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bits != 0u) __hip_atomic_fetch_or(&R.agg->status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {                  // (fields no atomic above touches)
    Ctl* g = R.agg;
    g->idx_y0 = 0; g->idx_y1 = 1;
    for (int j = 0; j < kMaxK; ++j) g->idx_k[j] = 2 + j;
    g->t0 = g->t1 = A.n_out > 0 ? cp.t_out[A.n_out - 1] : A.t0;
    g->done = 1;
  }
}

// the instantiations persist_fn offers for the shared kernel: S = 6 with and without the tsit5 dense output, S = 3, S = 13 FSAL
// shaped (dopri8), S = 1 not FSAL shaped (adaptive_heun)
template <typename T, class RHS>
struct RowsKernels {
  static const void* fn(int S, int ts_dense, int fsal) {
    if (S == 6 && fsal) return ts_dense ? (const void*)k_rows_rowlocal<T, 6, true, RHS> : (const void*)k_rows_rowlocal<T, 6, false, RHS>;
    if (S == 3 && fsal && !ts_dense) return (const void*)k_rows_rowlocal<T, 3, false, RHS>;
    if (S == 13 && fsal && !ts_dense) return (const void*)k_rows_rowlocal<T, 13, false, RHS, true>;
    if (S == 1 && !fsal && !ts_dense) return (const void*)k_rows_rowlocal<T, 1, false, RHS, false>;
    return nullptr;
  }
};

}  // namespace mi

// the catalogue families' kernels, one translation unit per state dtype (mi_ode_rows.hip, mi_ode_rows_f32.hip)
const void* mi_rows_fn_f64(int family, int S, int ts_dense, int fsal);
const void* mi_rows_fn_f32(int family, int S, int ts_dense, int fsal);
// host helpers the per-trajectory entry points share (mi_ode_rows.hip): the handle's staging arrays for n output times, and its tableau,
// right-hand side and controller parameters as the kernels get them
struct mi_ode_solver;
int mi_rows_ensure_t_out(mi_ode_solver* h, int n);
void mi_rows_step_args(mi_ode_solver* h, mi::StepArgs& A);
