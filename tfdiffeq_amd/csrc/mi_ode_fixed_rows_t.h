// Fixed-grid solves (euler, rk4) with PER-ROW output times and lengths: a 2-D `t` [batch, T] and options['t_lengths'] with a fixed-grid
// method / mi_ode_integrate_fixed_rows_t.
//
// k_fixed_rowlocal (mi_ode_step_fused.h) hands every lane the same grid.  Here every lane builds its own view of the call
//   t_row = t + row * T,   len = len[row] (clamped to 1 .. T)
// and walks its trajectory over its own times: step n goes from (T)t_row[n] to (T)t_row[n + 1] and writes solution[n + 1].  On the default
// grid every step ends on a requested time, so nothing is interpolated.  Row i is what k_fixed_rowlocal returns for
// (y0[i:i+1], t[i, :len_i]), bit for bit: the same operations in the same order (Euler: fixed_grid.py:6-7, RK4 3/8 rule:
// rk_common.py:73-81, true divisions included), under the project's -ffp-contract=off.
//   * fixed_rows_walk: one trajectory, no HIP construct (the CPU tests compile it with g++);
//   * the geometry of the non-cooperative branch of k_fixed_rowlocal: one trajectory per lane, 256-thread workgroups, any batch; no
//     barrier, no LDS; every loop is bounded by T, so whatever the times hold - unordered values, NaN - a lane reads inside its row of
//     t, writes inside its column of the solution and stops: with wrong numbers, never with an access outside the row;
//   * solution[k, row] for k >= len[row] is written as exact zeros by the lane after its walk; t[row, len[row]:] is never read.
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

// D elements of one trajectory as one vector access where the row's size allows it (as RowVec of mi_ode_stage_rowlocal.h)
template <typename T, int D>
struct alignas((D * sizeof(T)) % 16 == 0 ? 16 : ((D * sizeof(T)) % 8 == 0 ? 8 : sizeof(T))) FixedRowVec {
  T v[D];
};

// One trajectory over its own times.  t_row: the row's len times, float64 (values already rounded to the state dtype); y: y0 on entry,
// the last state on exit; out: the row's column of the solution, out + k * plane is solution[k] (the caller has written solution[0]).
template <typename T, int D, class RHS>
MI_ODE_ROW_HD void fixed_rows_walk(const RHS& rhs, T sign, int rk4, const double* t_row, int len, FixedRowVec<T, D>& y, T* out, long long plane) {
  using Row = FixedRowVec<T, D>;
  for (int n = 0; n + 1 < len; ++n) {
    const T t0 = (T)t_row[n];                                // solvers.py:84: the grid is cast to the STATE dtype
    const T t1 = (T)t_row[n + 1];
    const T dt = t1 - t0;
    const T te = t0 + (T)0;                                  // fixed_grid.py:7: t + eps, eps == 0 on this route
    T k1[D], k2[D], k3[D], k4[D], ys[D];
    Row yn;
    rhs(sign * te, y.v, k1);
#pragma unroll
    for (int d = 0; d < D; ++d) k1[d] = sign * k1[d];
    if (!rk4) {
#pragma unroll
      for (int d = 0; d < D; ++d) yn.v[d] = y.v[d] + dt * k1[d];                       // fixed_grid.py:7
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) ys[d] = y.v[d] + dt * k1[d] / (T)3;                 // rk_common.py:77
      rhs(sign * (te + dt / (T)3), ys, k2);
#pragma unroll
      for (int d = 0; d < D; ++d) { k2[d] = sign * k2[d]; ys[d] = y.v[d] + dt * (k1[d] / (T)-3 + k2[d]); }   // :78
      rhs(sign * (te + dt * (T)2 / (T)3), ys, k3);
#pragma unroll
      for (int d = 0; d < D; ++d) { k3[d] = sign * k3[d]; ys[d] = y.v[d] + dt * (k1[d] - k2[d] + k3[d]); }   // :79
      rhs(sign * (te + dt), ys, k4);
#pragma unroll
      for (int d = 0; d < D; ++d) {
        k4[d] = sign * k4[d];
        yn.v[d] = y.v[d] + (k1[d] + (T)3 * k2[d] + (T)3 * k3[d] + k4[d]) * (dt / (T)8);                       // :81
      }
    }
    *(Row*)(out + (long long)(n + 1) * plane) = yn;          // solvers.py:97-100 on a grid hit: exactly y1
    y = yn;
  }
}

}  // namespace mi

#if defined(__HIPCC__)
#include "mi_ode_stage_rowlocal.h"

#define MI_ODE_FIXED_ROWS_T_PLUGIN_ABI 1

// what a fixed-rows-t plugin exports (mi_ode_fixed_rows_t_plugin.h): the k_fixed_rowlocal_t instantiation of a user's functor
struct mi_ode_fixed_rows_t_plugin {
  int abi;                     // MI_ODE_FIXED_ROWS_T_PLUGIN_ABI
  int dtype;                   // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int reserved;
  const void* fixed_rows_t_fn; // k_fixed_rowlocal_t<T, RHS>
};

namespace mi {

struct FixedRowsTArgs {
  const void* y0;              // [batch, D]
  void* out;                   // [T, batch * D]
  const double* t;             // device [batch][T]: row i's times are t[i][0 .. len[i] - 1], strictly increasing
  const int* len;              // device [batch], values 1 .. T; null: every row has T times
  long long batch;
  int T;
  int rk4;                     // 0: Euler, 1: RK4 (3/8 rule)
  RhsParams rhs;
};

template <typename T, class RHS>
__global__ __launch_bounds__(256) void k_fixed_rowlocal_t(FixedRowsTArgs A) {
  static_assert(!rhs_is_coop<RHS>::value, "a cooperative right-hand side has barriers inside f: never under per-lane control flow");
  constexpr int D = RHS::D;
  using Row = FixedRowVec<T, D>;
  const RHS rhs(A.rhs);
  const T sign = (T)A.rhs.sign;
  const long long plane = A.batch * D;                       // elements per solution row
  const T* y0p = (const T*)A.y0;
  T* out = (T*)A.out;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < A.batch; row += (long long)gridDim.x * blockDim.x) {
    const long long e0 = row * D;
    // the lane's own view of the call
    const double* t_row = A.t + row * A.T;
    int len = A.len != nullptr ? A.len[row] : A.T;
    len = len < 1 ? 1 : (len > A.T ? A.T : len);             // (the host refuses such a length; no read or write outside the row either way)
    Row y = *(const Row*)(y0p + e0);
    *(Row*)(out + e0) = y;                                   // solution = [y0]
    fixed_rows_walk<T, D, RHS>(rhs, sign, A.rk4, t_row, len, y, out + e0, plane);
    Row z;                                                   // the padding of a short row: exact zeros
#pragma unroll
    for (int d = 0; d < D; ++d) z.v[d] = (T)0;
    for (int k = len; k < A.T; ++k) *(Row*)(out + (long long)k * plane + e0) = z;
  }
}

}  // namespace mi

// the catalogue families' kernels, one translation unit per state dtype (mi_ode_fixed_rows_t.hip, mi_ode_fixed_rows_t_f32.hip)
const void* mi_fixed_rows_t_fn_f64(int family);
const void* mi_fixed_rows_t_fn_f32(int family);
#endif  // __HIPCC__
