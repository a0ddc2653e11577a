"""Systems, inputs and generated sources of the per-trajectory step control tests (options={'per_trajectory': True}, csrc/mi_ode_rows.h) -
shared by the CPU tests (refusals, plan, the per-row integration compiled by g++), the GPU tests and `__graft_entry__.build()`, which
compiles the rows plugins here so that the GPU box does not run hipcc."""
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, 'tests')):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

DTYPES = (torch.float64, torch.float32)


# ---- right-hand sides ---------------------------------------------------------------------------------------------------------------
def van_der_pol():
    from tfdiffeq_amd import plugin_examples
    return plugin_examples.van_der_pol()                 # rhs.CustomRowLocal, dim 2 (mu = 5)


def blow_up():
    """y' = y^2: y(t) = y0 / (1 - y0 t) leaves every float at t = 1 / y0."""
    from tfdiffeq_amd import rhs
    return rhs.CustomRowLocal(1, "k[0] = y[0] * y[0];", torch_fn=lambda t, y: y * y)


def time_callable(t, y):
    """A plain Python callable of 4 elements per trajectory that uses t: lowered to a row program (tfdiffeq_amd/lower.py)."""
    return torch.sin(y) * t - 0.5 * y + torch.cos(t)


TIME_DIM = 4


def lorenz_np(t, y, s=10., b=8. / 3., r=28.):
    return np.stack([s * (y[..., 1] - y[..., 0]), y[..., 0] * (r - y[..., 2]) - y[..., 1], y[..., 0] * y[..., 1] - b * y[..., 2]], axis=-1)


def lv_np(t, y, a=1.5, b=1.0, c=3.0, d=1.0):
    u, v = y[..., 0], y[..., 1]
    return np.stack([a * u - b * u * v, -c * v + d * u * v], axis=-1)


def vdp_np(t, y, mu=5.0):
    return np.stack([y[..., 1], mu * (1 - y[..., 0] * y[..., 0]) * y[..., 1] - y[..., 0]], axis=-1)


def time_np(t, y):
    return np.sin(y) * t - 0.5 * y + np.cos(t)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def base_y0():
    """70 Lorenz rows spread over 3.3 decades: one full wavefront, one with 6 live lanes, a dead remainder of the workgroup."""
    return torch.tensor(np.random.RandomState(0).randn(70, 3) * 10 ** np.linspace(-2, 1.3, 70)[:, None])


BASE_T = np.linspace(0., 1., 5)
BASE_ROWS = (0, 10, 35, 63, 64, 69)


def lv_y0(n=9):
    """Lotka-Volterra rows from near the fixed point's scale to well away from it (positive quadrant)."""
    g = torch.Generator().manual_seed(1)
    return (0.2 + torch.rand(n, 2, generator=g, dtype=torch.float64)) * (10 ** torch.linspace(-1, 0.7, n, dtype=torch.float64))[:, None]


# ---- sources build() compiles ---------------------------------------------------------------------------------------------------------
def rows_sources(device='cpu'):
    """The row-local AND the rows plugin of every plugin system the tests use (a rows call creates its handle from the row-local one)."""
    from tfdiffeq_amd import lower, rhs
    out = []
    for dt in DTYPES:
        for system in (van_der_pol(), blow_up()):
            out += [system.source(dt), system.rows_source(dt)]
        for src in lower.sources_for(time_callable, torch.zeros(2, TIME_DIM, dtype=dt, device=device)):
            out += [src, rhs.rows_source_of(src)]
    return out


# ---- the per-row integration as host code ----------------------------------------------------------------------------------------------
def _between(text, start, end):
    a = text.index(start)
    return text[a:text.index(end, a)]


HOST_PRELUDE = r"""
// (compiled with an include directory that holds an empty hip/hip_runtime.h)
// host stand-ins for what csrc/mi_ode_dev.h, mi_ode_dense.h and mi_ode_ctrl_dev.h use of HIP (none of it is reached by one row's integration)
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
using std::isnan; using std::isinf;
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __HIP_MEMORY_SCOPE_SYSTEM 0
#define __HIP_MEMORY_SCOPE_WORKGROUP 0
template <class P> auto __hip_atomic_load(P* p, int, int) { return *p; }
template <class P, class V> void __hip_atomic_store(P* p, V v, int, int) { *p = v; }
struct mi_host_dim3 { unsigned x = 0, y = 0, z = 0; };
static mi_host_dim3 threadIdx, blockIdx, blockDim, gridDim;
inline void __syncthreads() {}
template <class V> V __shfl_down(V v, int, int) { return v; }
"""


def host_source(functor, dim):
    """A g++ translation unit: the project's own device headers behind host stand-ins for the HIP names they mention, the per-element step
    functions cut out of csrc/mi_ode_step_fused.h verbatim (that header also holds the matrix-core kernels), csrc/mi_ode_rows_core.h, and
    `rows_run_<S>` entry points around `functor` (C++ text of `template <typename T> struct Rhs` with D = dim)."""
    csrc = os.path.join(ROOT, 'tfdiffeq_amd', 'csrc')
    fused = open(os.path.join(csrc, 'mi_ode_step_fused.h')).read()
    step_args = _between(fused, 'struct StepArgs {', '};') + '};\n'
    step_planes = _between(fused, 'template <typename T, int S>\nstruct StepPlanes {', '};') + '};\n'
    per_element = _between(fused, '// stages 1..S at compile time', '// ----')
    assert 'step_combine' in per_element and 'step_emit' in per_element and 'step_finish' in per_element and 'step_y1_general' in per_element
    return HOST_PRELUDE + r"""
#include "mi_ode_dev.h"
#include "mi_ode_dense.h"
#include "mi_ode_ctrl_dev.h"
namespace mi {
%s
%s
%s
}
#include "mi_ode_rows_core.h"
namespace mi {
%s
}
using namespace mi;
// tab: alpha[13], beta[13][13], c_sol[14], c_error[14], c_mid[14]; ctrl: rtol, atol, safety, ifactor, dfactor, first_step (nan: auto), max_num_steps, order,
// init_order, controller, interp; out: [n_out][batch * D] (solution[1:]); stats: [batch][4]
template <int S, bool TS, bool FSAL>
static void run(const double* tab, const double* ctrl, const double* rhs_scalars, long long batch, const double* y0, const double* t, int T, double* out,
                long long* stats) {
  constexpr int D = %d;
  StepArgs sa;
  memset(&sa, 0, sizeof(sa));
  const double* p = tab;
  for (int i = 0; i < 13; ++i) sa.alpha[i] = *p++;
  for (int i = 0; i < 13; ++i) for (int j = 0; j < 13; ++j) sa.beta[i][j] = *p++;
  for (int j = 0; j < 14; ++j) sa.csol[j] = *p++;
  for (int j = 0; j < 14; ++j) sa.e[j] = *p++;
  for (int j = 0; j < 14; ++j) sa.cmid[j] = *p++;
  for (int i = 0; i < 8; ++i) sa.rhs.s[i] = rhs_scalars[i];
  sa.rhs.sign = 1.0;
  sa.batch = batch; sa.dim = D; sa.n_plane = batch * D; sa.out = out; sa.interp = (int)ctrl[10];
  CtrlParams cp;
  memset(&cp, 0, sizeof(cp));
  cp.rtol = ctrl[0]; cp.atol = ctrl[1]; cp.safety = ctrl[2]; cp.ifactor = ctrl[3]; cp.dfactor = ctrl[4];
  cp.inv_ifactor = 1.0 / cp.ifactor; cp.inv_dfactor = 1.0 / cp.dfactor;
  cp.auto_first_step = std::isnan(ctrl[5]) ? 1 : 0;
  cp.max_num_steps = (long long)ctrl[6]; cp.order = (int)ctrl[7]; cp.init_order = (int)ctrl[8]; cp.controller = (int)ctrl[9];
  cp.is_f32 = 0; cp.n_stages = S; cp.n_local = D; cp.t_out = t + 1;
  sa.cp = cp; sa.t_out = t + 1;
  const Rhs<double> rhs(sa.rhs);
  for (long long row = 0; row < batch; ++row) {
    double y[D], f[D];
    for (int d = 0; d < D; ++d) y[d] = y0[row * D + d];
    RowResult res;
    rows_integrate<double, S, TS, FSAL, Rhs<double>>(rhs, sa, cp, 1.0, t[0], cp.auto_first_step ? 0.0 : ctrl[5], T - 1, y, f, row * D, res);
    stats[row * 4 + 0] = res.n_attempt; stats[row * 4 + 1] = res.n_accept; stats[row * 4 + 2] = res.nfe; stats[row * 4 + 3] = (long long)res.status;
  }
}
extern "C" int rows_run(int S, int ts, int fsal, const double* tab, const double* ctrl, const double* rhs_scalars, long long batch, const double* y0,
                        const double* t, int T, double* out, long long* stats) {
  if (S == 6 && fsal && !ts) run<6, false, true>(tab, ctrl, rhs_scalars, batch, y0, t, T, out, stats);
  else if (S == 6 && fsal && ts) run<6, true, true>(tab, ctrl, rhs_scalars, batch, y0, t, T, out, stats);
  else if (S == 3 && fsal) run<3, false, true>(tab, ctrl, rhs_scalars, batch, y0, t, T, out, stats);
  else if (S == 13 && fsal) run<13, false, true>(tab, ctrl, rhs_scalars, batch, y0, t, T, out, stats);
  else if (S == 1 && !fsal) run<1, false, false>(tab, ctrl, rhs_scalars, batch, y0, t, T, out, stats);
  else return -1;
  return 0;
}
""" % (step_args, step_planes, per_element, functor, dim)


LORENZ_FUNCTOR = _between(open(os.path.join(ROOT, 'tfdiffeq_amd', 'csrc', 'mi_ode_stage_rowlocal.h')).read(),
                          '// Lorenz, examples/lorenz_attractor.py:28-37', 'template <typename T, int D>').replace('RhsLorenz', 'Rhs')
LV_FUNCTOR = _between(open(os.path.join(ROOT, 'tfdiffeq_amd', 'csrc', 'mi_ode_stage_rowlocal.h')).read(),
                      '// Lotka-Volterra, examples/ode_usage.ipynb', '// Lorenz, examples/lorenz_attractor.py:28-37').replace('RhsLotkaVolterra', 'Rhs')


def tableau_array(tb, c_mid):
    a = np.zeros(13 + 13 * 13 + 3 * 14)
    S = len(tb.alpha)
    a[:S] = tb.alpha
    for i, row in enumerate(tb.beta):
        a[13 + 13 * i:13 + 13 * i + len(row)] = row
    o = 13 + 13 * 13
    a[o:o + len(tb.c_sol)] = tb.c_sol
    a[o + 14:o + 14 + len(tb.c_error)] = tb.c_error
    if c_mid is not None:
        a[o + 28:o + 28 + len(c_mid)] = c_mid
    return a
