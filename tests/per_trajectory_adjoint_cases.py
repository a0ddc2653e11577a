"""Systems, inputs, oracle and generated sources of the per-trajectory adjoint tests (odeint_adjoint with options={'per_trajectory': True},
csrc/mi_ode_rows_adjoint.h) - shared by the CPU tests (refusals, plan, the t rule, one row's whole backward compiled by g++), the GPU tests
and `__graft_entry__.build()`, which compiles the rows-adjoint plugins (and the forward's row-local / rows plugins) here so that the GPU
box does not run hipcc.

Every system is a torch.nn.Module with a numpy twin of its AUGMENTED dynamics (adjoint.py:69-105) with hand-written Jacobians: the oracle
(`oracle_backward`) is the reference's adjoint algorithm on one trajectory, every interval an `oracle.ode_numpy.odeint` call on the
four-component tuple (y [1, D], adj_y [1, D], adj_t [], adj_params [P]) - which already does per-component control."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, 'tests')):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import per_trajectory_cases as PC                         # noqa: E402

DTYPES = (torch.float64, torch.float32)
METHODS = ('dopri5', 'bosh3')
ON = {'per_trajectory': True}


# ---- systems ------------------------------------------------------------------------------------------------------------------------
class LorenzModule(torch.nn.Module):
    """D = 3, P = 3 (sigma, rho, beta as 0-d parameters), N_aug = 10."""

    def __init__(self, dtype=torch.float64, device='cpu', values=(10., 28., 8. / 3.)):
        super(LorenzModule, self).__init__()
        self.sigma, self.rho, self.beta = (torch.nn.Parameter(torch.tensor(v, dtype=torch.float64).to(device=device, dtype=dtype)) for v in values)

    def forward(self, t, y):
        x, u, z = y[..., 0], y[..., 1], y[..., 2]
        return torch.stack([self.sigma * (u - x), x * (self.rho - z) - u, x * u - self.beta * z], dim=-1)


def lorenz_f_np(th, t, y):
    s, r, b = th
    return np.stack([s * (y[..., 1] - y[..., 0]), y[..., 0] * (r - y[..., 2]) - y[..., 1], y[..., 0] * y[..., 1] - b * y[..., 2]], axis=-1)


def lorenz_aug_np(th):
    s, r, b = th

    def aug(t, z):
        y, a = z[0], z[1]
        x, u, w = y[..., 0], y[..., 1], y[..., 2]
        a0, a1, a2 = a[..., 0], a[..., 1], a[..., 2]
        vy = -np.stack([a0 * (-s) + a1 * (r - w) + a2 * u, a0 * s - a1 + a2 * x, -a1 * x - a2 * b], axis=-1)
        vth = -np.stack([np.sum(a0 * (u - x)), np.sum(a1 * x), np.sum(-a2 * w)])
        return (lorenz_f_np(th, t, y), vy, np.zeros_like(z[2]), vth.astype(y.dtype))
    return aug


class TimeModule(torch.nn.Module):
    """tests/discrete_lowered_cases.scalars as a Module: f = a sin(y w) t - c y + cos(t).  D = 3, P = 4 (a 0-d, c [3]), w a constant; its
    df/dt is not zero, so the adj_t component takes part in the control."""

    def __init__(self, dtype=torch.float64, device='cpu', seed=0):
        super(TimeModule, self).__init__()
        g = torch.Generator().manual_seed(400 + seed)
        self.a = torch.nn.Parameter(torch.tensor(0.8, dtype=torch.float64).to(device=device, dtype=dtype))
        self.c = torch.nn.Parameter((torch.tensor([0.5, 0.3, 0.7], dtype=torch.float64) + 0.05 * torch.randn(3, generator=g, dtype=torch.float64)).to(device=device, dtype=dtype))
        self.register_buffer('w', (1.0 + 0.2 * torch.randn(3, generator=g, dtype=torch.float64)).to(device=device, dtype=dtype))

    def forward(self, t, y):
        return self.a * torch.sin(y * self.w) * t - self.c * y + torch.cos(t)


def time_theta(mod):
    return (float(mod.a.detach()), mod.c.detach().cpu().double().numpy().copy(), mod.w.detach().cpu().double().numpy().copy())


def time_f_np(th, t, y):
    a, c, w = th
    dt = y.dtype.type
    return dt(a) * np.sin(y * w.astype(y.dtype)) * t - c.astype(y.dtype) * y + np.cos(t)


def time_aug_np(th):
    a, c, w = th

    def aug(t, z):
        y, adj = z[0], z[1]
        dt = y.dtype
        A, cc, ww = dt.type(a), c.astype(dt), w.astype(dt)
        sn, cs = np.sin(y * ww), np.cos(y * ww)
        vy = -(adj * (A * ww * cs * t - cc))
        vt = -np.sum(adj * (A * sn - np.sin(t)))
        va = -np.sum(adj * sn * t)
        vc = (adj * y).reshape(-1)
        return (time_f_np(th, t, y), vy, np.asarray(vt, dtype=dt), np.concatenate([[va], vc]).astype(dt))
    return aug


def time_y0(n=9):
    """9 rows spread over 1.5 decades."""
    g = torch.Generator().manual_seed(7)
    return torch.randn(n, 3, generator=g, dtype=torch.float64) * (10 ** torch.linspace(-1, 0.5, n, dtype=torch.float64))[:, None]


TIME_T = np.linspace(0.2, 1.7, 4)


def lorenz_theta(mod):
    return tuple(float(p_.detach()) for p_ in (mod.sigma, mod.rho, mod.beta))


SYSTEMS = {
    # name: (module class, theta of a module, f twin, augmented twin, y0, t)
    'lorenz': (LorenzModule, lorenz_theta, lorenz_f_np, lorenz_aug_np, PC.base_y0, PC.BASE_T),
    'time': (TimeModule, time_theta, time_f_np, time_aug_np, time_y0, TIME_T),
}


# ---- the oracle: the reference's adjoint algorithm on ONE trajectory ------------------------------------------------------------------
def oracle_backward(name, theta, t, ans_row, g_row, rtol, atol, method, max_num_steps=2 ** 31 - 1):
    """ans_row / g_row: [T, D] numpy arrays of ONE trajectory in the dtype to compute in.  Returns grad_y0 [D], grad_params [P],
    time_vjps [T], and [T - 1] lists of attempts / accepted / nfe (index k - 1: the interval t_k -> t_{k-1})."""
    from oracle import ode_numpy as O
    f_np, aug_np = SYSTEMS[name][2], SYSTEMS[name][3]
    dt = ans_row.dtype
    T = ans_row.shape[0]
    aug = aug_np(theta)
    n_par = {'lorenz': 3, 'time': 4}[name]
    adj_y = g_row[T - 1][None].copy()
    adj_t = np.zeros((), dtype=dt)
    adj_p = np.zeros(n_par, dtype=dt)
    tv = np.zeros(T, dtype=dt)
    att, acc, nfe = [0] * (T - 1), [0] * (T - 1), [0] * (T - 1)
    for k in range(T - 1, 0, -1):
        y = ans_row[k][None]
        f = f_np(theta, dt.type(t[k]), y)
        dl = f[0, 0] * g_row[k][0]
        for d in range(1, f.shape[1]):
            dl = dl + f[0, d] * g_row[k][d]
        adj_t = (adj_t - dl).astype(dt)
        tv[k] = dl
        sol, st = O.odeint(aug, (y, adj_y, adj_t, adj_p), np.array([t[k], t[k - 1]]), rtol=rtol, atol=atol, method=method,
                           options={'max_num_steps': max_num_steps}, return_stats=True)
        att[k - 1], acc[k - 1], nfe[k - 1] = st.n_attempts, st.n_accepted, st.nfe
        adj_y = sol[1][1] + g_row[k - 1][None]
        adj_t, adj_p = sol[2][1], sol[3][1]
    tv[0] = adj_t
    return adj_y[0], adj_p, tv, att, acc, nfe


def oracle_forward(name, theta, y0, t, rtol, atol, method):
    """[T, batch, D]: every row its own solve."""
    from oracle import ode_numpy as O
    f_np = SYSTEMS[name][2]
    return np.concatenate([O.odeint(lambda tt, y: f_np(theta, tt, y), y0[i:i + 1], t, rtol=rtol, atol=atol, method=method) for i in range(y0.shape[0])], axis=1)


def cotangent(ans, every=True):
    """The gradient of a fixed loss with respect to the solution: sum(sin(ans) * weights) over every output time (the jumps
    adj_y += g are exercised) or over the last one only."""
    w = np.cos(np.arange(ans.size, dtype=np.float64).reshape(ans.shape) * 0.37).astype(ans.dtype)
    g = np.cos(ans) * w
    if not every:
        g[:-1] = 0
    return g


# ---- sources build() compiles ---------------------------------------------------------------------------------------------------------
def modules(device='cpu'):
    out = []
    for dt in DTYPES:
        out.append((LorenzModule(dt, device), torch.zeros(2, 3, dtype=dt, device=device)))
        out.append((TimeModule(dt, device), torch.zeros(2, 3, dtype=dt, device=device)))
    return out


def adjoint_sources(device='cpu'):
    """The rows-adjoint plugin of every system of the tests, and the row-local and rows plugins its forward runs on."""
    from tfdiffeq_amd import lower, rhs
    out = []
    for mod, y0 in modules(device):
        tr = lower.trace(mod, y0)
        for src in lower.sources_for(mod, y0):
            out += [src, rhs.rows_source_of(src)]
        out.append(lower.adjoint_source(tr))
    return out


# ---- one row's whole backward as host code ----------------------------------------------------------------------------------------------
def host_source(tr):
    """A g++ translation unit: the device headers behind per_trajectory_cases' host stand-ins, the per-element step functions cut out of
    csrc/mi_ode_step_fused.h, csrc/mi_ode_rows_core.h, csrc/mi_ode_rows_adjoint_core.h, the generated functor (lower.host_vjp_t_source) and
    `adj_rows_run` around rows_adjoint_row."""
    from tfdiffeq_amd import lower
    csrc = os.path.join(ROOT, 'tfdiffeq_amd', 'csrc')
    fused = open(os.path.join(csrc, 'mi_ode_step_fused.h')).read()
    step_args = PC._between(fused, 'struct StepArgs {', '};') + '};\n'
    step_planes = PC._between(fused, 'template <typename T, int S>\nstruct StepPlanes {', '};') + '};\n'
    per_element = PC._between(fused, '// stages 1..S at compile time', '// ----')
    return PC.HOST_PRELUDE + r"""
#include "mi_ode_dev.h"
#include "mi_ode_dense.h"
#include "mi_ode_ctrl_dev.h"
namespace mi {
%s
%s
%s
}
#include "mi_ode_rows_core.h"
#include "mi_ode_rows_adjoint_core.h"
%s
using namespace mi;
// tab: as per_trajectory_cases.tableau_array; ctrl: rtol, atol, safety, ifactor, dfactor, max_num_steps, order, init_order
template <int S>
static void run(const double* tab, const double* ctrl, const double* ps, const double* cw, long long batch, int T, const double* t,
                const double* ans, const double* g, double* gy0, double* rowp, double* rowt, long long* counts, long long* status) {
  using R = RhsUser<double>;
  using L = AdjLayout<R>;
  StepArgs sa;
  memset(&sa, 0, sizeof(sa));
  const double* p = tab;
  for (int i = 0; i < 13; ++i) sa.alpha[i] = *p++;
  for (int i = 0; i < 13; ++i) for (int j = 0; j < 13; ++j) sa.beta[i][j] = *p++;
  for (int j = 0; j < 14; ++j) sa.csol[j] = *p++;
  for (int j = 0; j < 14; ++j) sa.e[j] = *p++;
  for (int j = 0; j < 14; ++j) sa.cmid[j] = *p++;
  sa.batch = batch; sa.dim = L::D; sa.n_plane = batch * L::D; sa.interp = MI_ODE_INTERP_QUARTIC_MID;
  CtrlParams cp;
  memset(&cp, 0, sizeof(cp));
  cp.rtol = ctrl[0]; cp.atol = ctrl[1]; cp.safety = ctrl[2]; cp.ifactor = ctrl[3]; cp.dfactor = ctrl[4];
  cp.inv_ifactor = 1.0 / cp.ifactor; cp.inv_dfactor = 1.0 / cp.dfactor;
  cp.auto_first_step = 1;
  cp.max_num_steps = (long long)ctrl[5]; cp.order = (int)ctrl[6]; cp.init_order = (int)ctrl[7]; cp.controller = MI_ODE_CTRL_MISC;
  cp.is_f32 = 0; cp.n_stages = S; cp.n_local = L::D;
  double neg_t[64];
  for (int i = 0; i < T; ++i) neg_t[i] = -t[i];
  const R rhs(ps, cw);
  for (long long row = 0; row < batch; ++row) {
    AdjRowIO<double> io;
    io.ans = ans + row * L::D; io.g = g + row * L::D; io.plane = batch * L::D;
    io.grad_y0 = gy0 + row * L::D; io.grad_params = rowp + row * L::PP; io.time_vjps = rowt + row * T;
    io.counts = counts + row * 3 * (T - 1);
    status[row] = (long long)rows_adjoint_row<double, S, R>(rhs, sa, cp, neg_t, T, io);
  }
}
extern "C" int adj_rows_run(int S, const double* tab, const double* ctrl, const double* ps, const double* cw, long long batch, int T, const double* t,
                            const double* ans, const double* g, double* gy0, double* rowp, double* rowt, long long* counts, long long* status) {
  if (T > 64) return -1;
  if (S == 6) run<6>(tab, ctrl, ps, cw, batch, T, t, ans, g, gy0, rowp, rowt, counts, status);
  else if (S == 3) run<3>(tab, ctrl, ps, cw, batch, T, t, ans, g, gy0, rowp, rowt, counts, status);
  else return -1;
  return 0;
}
""" % (step_args, step_planes, per_element, lower.host_vjp_t_source(tr))


def host_constants(tr):
    """(pool, ps) of a trace for the host functor: the tensors it closes over in one float64 array, its first 8 Python floats."""
    from tfdiffeq_amd import lower
    lay = lower.Layout(tr)
    pool = np.zeros(max(lay.size, 1))
    for idx, off in enumerate(lay.tensor_off):
        x = tr.tensors[idx]['t'].detach()
        pool[off:off + x.numel()] = x.reshape(-1).double().cpu().numpy()
    pool[lay.extra_off:lay.extra_off + max(len(tr.scalars) - 8, 0)] = np.asarray(tr.scalars[8:])
    ps = (C.c_double * 8)(*(list(tr.scalars[:8]) + [0.0] * (8 - len(tr.scalars[:8]))))
    return pool, ps


def compact_order(tr, params):
    """For every parameter of the module (in module order) its slice of the trace's compact parameter vector."""
    from tfdiffeq_amd import lower
    plist, _n = lower.vjp_params(tr)
    out = []
    for p_ in params:
        hit = [(off, n) for idx, off, n in plist if tr.tensors[idx]['t'] is p_]
        assert len(hit) == 1
        out.append(hit[0])
    return out
