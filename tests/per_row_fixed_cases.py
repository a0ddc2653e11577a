"""Systems, inputs and generated sources of the tests of fixed-grid solves and exact gradients on every row's own time grid (a 2-D `t`
and options['t_lengths'] with euler / rk4; csrc/mi_ode_fixed_rows_t.h, csrc/mi_ode_discrete_row_t.h) - shared by the CPU tests, the GPU
tests and `__graft_entry__.build()`, which compiles the fixed-rows-t and discrete-t plugins here so that the GPU box does not run hipcc.
The systems are those of tests/per_trajectory_cases.py (forward) and tests/discrete_lowered_cases.py (backward)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, 'tests')):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import discrete_lowered_cases as DC                         # noqa: E402
import per_row_times_cases as RC                            # noqa: E402
import per_trajectory_cases as PC                           # noqa: E402

DTYPES = PC.DTYPES
METHODS = ('euler', 'rk4')
BACKWARD = ('scalars', 'spiral', 'tanh8')                   # the systems of DC.SYSTEMS with a [batch, dim] state


def mixed_lengths(batch, T):
    """Lengths 1, 2 and T next to each other in every wavefront: the wave-uniform trip count of the backward kernel."""
    return np.array([(1, 2, T)[i % 3] for i in range(batch)], dtype=np.int32)


def ragged_with(lengths, T, end=1.0):
    """RC.ragged's times for given lengths: row i has len_i times linspace(0, end_i, len_i), NaN in the padding."""
    batch = len(lengths)
    t = np.full((batch, T), np.nan)
    for i, n in enumerate(lengths):
        t[i, :n] = np.linspace(0., end * (0.5 + 0.5 * i / max(batch - 1, 1)), n) if n > 1 else 0.
    return t


# ---- one trajectory's walk and one row's reverse sweep as host code --------------------------------------------------------------------
HOST_WALK_ENTRY = r"""
#include "mi_ode_dev.h"
namespace mi {
%s
}
#include "mi_ode_fixed_rows_t.h"
using namespace mi;
// what a lane of k_fixed_rowlocal_t does, row after row: t: [batch][T]; len: [batch]; out: [T][batch * D]
template <typename T>
static void walk_rows(int rk4, const double* rhs_scalars, long long batch, const T* y0, const double* t, int Tn, const int* len, T* out) {
  constexpr int D = %d;
  RhsParams rp;
  memset(&rp, 0, sizeof(rp));
  for (int i = 0; i < 8; ++i) rp.s[i] = rhs_scalars[i];
  rp.sign = 1.0;
  const Rhs<T> rhs(rp);
  const long long plane = batch * D;
  for (long long row = 0; row < batch; ++row) {
    int n = len[row];
    n = n < 1 ? 1 : (n > Tn ? Tn : n);
    FixedRowVec<T, D> y;
    for (int d = 0; d < D; ++d) { y.v[d] = y0[row * D + d]; out[row * D + d] = y.v[d]; }
    fixed_rows_walk<T, D, Rhs<T>>(rhs, (T)1, rk4, t + row * Tn, n, y, out + row * D, plane);
    for (int k = n; k < Tn; ++k) for (int d = 0; d < D; ++d) out[(long long)k * plane + row * D + d] = (T)0;
  }
}
extern "C" int fixed_walk_f64(int rk4, const double* s, long long batch, const double* y0, const double* t, int T, const int* len, double* out) {
  walk_rows<double>(rk4, s, batch, y0, t, T, len, out); return 0;
}
extern "C" int fixed_walk_f32(int rk4, const double* s, long long batch, const float* y0, const double* t, int T, const int* len, float* out) {
  walk_rows<float>(rk4, s, batch, y0, t, T, len, out); return 0;
}
"""


def host_walk_source(functor, dim):
    """A g++ translation unit: csrc/mi_ode_dev.h behind PC.HOST_PRELUDE's stand-ins, `functor` (C++ text of `template <typename T> struct
    Rhs` with D = dim) and csrc/mi_ode_fixed_rows_t.h's fixed_rows_walk behind `fixed_walk_f64` / `fixed_walk_f32`."""
    return PC.HOST_PRELUDE + HOST_WALK_ENTRY % (functor, dim)


# ---- a lowered callable on the host: the forward walk and the masked reverse loop of a wavefront ---------------------------------------
HOST_LOWERED_ENTRY = r"""
// (appended to tfdiffeq_amd.lower.host_vjp_source: RhsUser<T> with operator() and vjp, constructed from (ps, cw))
#include <cstring>
#include "mi_ode_fixed_rows_t.h"
#include "mi_ode_discrete_row.h"
// what a lane of k_fixed_rowlocal_t does, row after row: t: [batch][T]; len: [batch]; out: [T][batch * D]
template <typename T>
static void walk_t_(int rk4, const double* ps, const T* cw, long long batch, const T* y0, const double* t, int Tn, const int* len, T* out) {
  constexpr int D = RhsUser<T>::D;
  const RhsUser<T> rhs(ps, cw);
  const long long plane = batch * D;
  for (long long row = 0; row < batch; ++row) {
    int n = len[row];
    n = n < 1 ? 1 : (n > Tn ? Tn : n);
    mi::FixedRowVec<T, D> y;
    for (int d = 0; d < D; ++d) { y.v[d] = y0[row * D + d]; out[row * D + d] = y.v[d]; }
    mi::fixed_rows_walk<T, D, RhsUser<T>>(rhs, (T)1, rk4, t + row * Tn, n, y, out + row * D, plane);
    for (int k = n; k < Tn; ++k) for (int d = 0; d < D; ++d) out[(long long)k * plane + row * D + d] = (T)0;
  }
}
extern "C" int walk_t_f64(int rk4, const double* ps, const double* cw, long long batch, const double* y0, const double* t, int T, const int* len, double* out) {
  walk_t_<double>(rk4, ps, cw, batch, y0, t, T, len, out); return 0;
}
extern "C" int walk_t_f32(int rk4, const double* ps, const float* cw, long long batch, const float* y0, const double* t, int T, const int* len, float* out) {
  walk_t_<float>(rk4, ps, cw, batch, y0, t, T, len, out); return 0;
}
// the sink of k_discrete_rowlocal_t without the butterfly: an inactive lane's contribution is masked to exactly 0
template <typename T> struct MaskSink {
  T* g;
  bool live;
  void add(int i, T v) { g[i] += live ? v : (T)0; }
};
// what a wavefront of k_discrete_rowlocal_t does, 64 rows at a time: the step loop runs down from the wavefront's largest length, every
// lane makes every call, a lane is active in step n only when it has a row and n <= len - 2
template <typename T, int S>
static void sweep_t_(const mi::DiscreteRowTableau& tb, int N, long long batch, const double* t, const int* len, const T* ys, const T* gys, T* gy0,
                     T* gtheta, const double* ps, const T* cw, long long* calls) {
  constexpr int D = RhsUser<T>::D;
  const RhsUser<T> f(ps, cw);
  MaskSink<T> acc{gtheta, false};
  const long long plane = batch * D;
  for (long long g0 = 0; g0 < batch; g0 += 64) {
    int ln[64], wlen = 1;
    bool live[64];
    T lam[64][D];
    for (int lane = 0; lane < 64; ++lane) {
      const long long row = g0 + lane;
      live[lane] = row < batch;
      int n = 1;
      if (live[lane]) { n = len != nullptr ? len[row] : N; n = n < 1 ? 1 : (n > N ? N : n); }
      ln[lane] = n;
      wlen = n > wlen ? n : wlen;
      for (int d = 0; d < D; ++d) lam[lane][d] = live[lane] ? gys[(long long)(n - 1) * plane + row * D + d] : (T)0;
    }
    for (int n = wlen - 2; n >= 0; --n)
      for (int lane = 0; lane < 64; ++lane) {
        const long long row = g0 + lane, e0 = row * D;
        const bool active = live[lane] && n <= ln[lane] - 2;
        acc.live = active;
        const T tn = active ? (T)t[row * N + n] : (T)0;
        const T h = active ? (T)t[row * N + n + 1] - tn : (T)0;
        T yn[D], lam2[D];
        for (int d = 0; d < D; ++d) yn[d] = active ? ys[(long long)n * plane + e0 + d] : (T)0;
        mi::discrete_row_step<T, S, D>(f, tb, yn, tn, h, lam[lane], lam2, acc);
        ++*calls;
        if (active) for (int d = 0; d < D; ++d) lam[lane][d] = lam2[d] + gys[(long long)n * plane + e0 + d];
      }
    for (int lane = 0; lane < 64; ++lane)
      if (live[lane]) for (int d = 0; d < D; ++d) gy0[(g0 + lane) * D + d] = lam[lane][d];
  }
}
extern "C" long long sweep_t_f64(int S, const double* a16, const double* b4, const double* c4, int N, long long batch, const double* t, const int* len,
                                 const double* ys, const double* gys, double* gy0, double* gtheta, const double* ps, const double* cw) {
  mi::DiscreteRowTableau tb;
  for (int i = 0; i < 4; ++i) {
    tb.b[i] = b4[i];
    tb.c[i] = c4[i];
    for (int j = 0; j < 4; ++j) tb.a[i][j] = a16[i * 4 + j];
  }
  long long calls = 0;
  if (S == 1) sweep_t_<double, 1>(tb, N, batch, t, len, ys, gys, gy0, gtheta, ps, cw, &calls);
  else if (S == 4) sweep_t_<double, 4>(tb, N, batch, t, len, ys, gys, gy0, gtheta, ps, cw, &calls);
  else return -1;
  return calls;
}
"""


def host_lowered_source(tr):
    """A g++ translation unit for a lowered row-local trace: lower.host_vjp_source (f and its generated vjp) with `walk_t_f64` /
    `walk_t_f32` around csrc/mi_ode_fixed_rows_t.h's fixed_rows_walk and `sweep_t_f64`, the masked loop of a wavefront of
    k_discrete_rowlocal_t over the unchanged discrete_row_step with a plain accumulator (compile with -I csrc)."""
    from tfdiffeq_amd import lower
    return lower.host_vjp_source(tr) + HOST_LOWERED_ENTRY


# ---- sources build() compiles ---------------------------------------------------------------------------------------------------------
def sources(device='cpu'):
    """Forward: the row-local AND the fixed-rows-t plugin of every plugin system the tests solve (the batch-of-one calls the rows are held to
    run on the row-local one).  Backward: for the systems of BACKWARD the same two of the forward solve, and the discrete-t plugin of the
    sweep (their discrete plugins: discrete_lowered_cases.discrete_sources)."""
    from tfdiffeq_amd import lower, rhs
    out = []
    for dt in DTYPES:
        system = PC.van_der_pol()
        out += [system.source(dt), system.fixed_rows_t_source(dt)]
        for method in METHODS:
            for src in lower.sources_for(PC.time_callable, torch.zeros(2, PC.TIME_DIM, dtype=dt, device=device), method=method):
                out += [src, rhs.fixed_rows_t_source_of(src)]
        for name in BACKWARD:
            f, _params, y0 = DC.SYSTEMS[name](device, dt)
            for method in METHODS:
                for src in lower.sources_for(f, y0.detach(), method=method):
                    out += [src, rhs.fixed_rows_t_source_of(src)]
            out.append(rhs.discrete_t_source_of(lower.discrete_source(lower.trace(f, y0))))
    uniq = []
    for src in out:
        if src not in uniq:
            uniq.append(src)
    return uniq
