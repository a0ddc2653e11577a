"""The fused hypersolver gradient as far as the CPU goes (csrc/mi_ode_hyper_grad.h, tfdiffeq_amd/hyper_solvers.py: describe_grad): the
yardstick of tests/hyper_grad_cases.py is sane (no gradient of the oracle is zero, the float32 bounds and the kink admissions hold), the
box function gives every limit its reason, the per-step reverse recursion - the host/device template the kernel instantiates - compiled by
g++ with a plain-loop dense g agrees with torch autograd at the float64 bound, the generated translation unit cross-compiles for gfx950, and
the C ABI gained the new entry point without a version change.  No GPU needed."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from torch import nn

from tests import hyper_cases as EC
from tests import hyper_grad_cases as GC
from tests import hyper_restatement as HR
from tfdiffeq_amd import _native as N
from tfdiffeq_amd import _plugin_build as PB
from tfdiffeq_amd import hyper_solvers as H
from tfdiffeq_amd import lower as L
from tfdiffeq_amd import rhs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', GC.CASES, ids=lambda c: c.name)
def test_oracle_gradients_are_non_zero_and_admissions_hold(case):
    out, grads, margin = GC.oracle(case)
    assert torch.isfinite(out).all()
    g = GC.make_g(case)
    y_leaf = GC.set_leaves(case, g)
    assert (grads['y0'] is not None) == y_leaf
    for p, gr in zip(g.parameters(), grads['params']):
        if case.cot == 'row0':                           # row 0 is the input itself: the loss does not depend on g
            assert gr is None or float(gr.abs().max()) == 0.0
            continue
        assert (gr is not None) == p.requires_grad
        if gr is not None:
            assert torch.isfinite(gr).all() and float(gr.abs().max()) > 0.0, 'a gradient of the oracle is zero: a kernel that returns zeros would pass'
    if y_leaf:
        assert float(grads['y0'].abs().max()) > 0.0
    if case.cot == 'row0':
        assert torch.equal(grads['y0'], torch.tensor(GC.cotangent_of(case)[0]))
    if GC.is_kinked(case):
        assert margin >= (GC.KINK_F32 if case.dtype == 'float32' else GC.KINK_F64), 'a pre-activation within %.1e of a kink' % margin
        if case.dtype == 'float32':
            assert case.B <= 4 and len(GC.GRIDS[case.grid]) <= 3 and max(case.hidden) <= 17
    if case.dtype == 'float32':
        e, b = GC.e32(case), GC.bound_of(case)
        floor = GC.bands.case_ceiling(GC.steps_of(case), stages=2 * GC.G_EVALS[case.op])
        print(case.name, 'E32 %.3e' % e, 'bound %.3e' % b)
        assert np.isfinite(e) and b == 4 * max(e, floor) and 1.6e-5 <= b < 1e-4, (case.name, e, b)


def test_the_cases_cover_what_the_issue_lists():
    cs = GC.CASES
    assert {1, 15, 16, 17, 37} <= set(c.B for c in cs)
    assert {1, 15, 16, 17, 50, 64, 127, 128} <= set(h for c in cs for h in c.hidden)
    assert set(len(c.hidden) + 1 for c in cs) >= {2, 3, 4}
    assert set(a for c in cs for a in c.acts) >= {'relu', 'leaky', 'prelu', 'prelu1', 'tanh', 'softplus', None}
    assert set(GC.dim_of(c) for c in cs) == {2, 3} and set(len(GC.GRIDS[c.grid]) for c in cs) <= {2, 3, 9}
    for dtype in ('float64', 'float32'):
        assert set(c.op for c in cs if c.dtype == dtype) == {'euler', 'midpoint', 'heun', 'gresid'}
    assert set(c.grad_grid for c in cs) == {0, 1, 2} and GC.BY_NAME['default_grid'].B == 16 * H.GRAD_DEFAULT_GRID + 5
    assert set(c.cot for c in cs) == {'all', 'last', 'row0', 'noncontig'} and set(c.leaves for c in cs) == {'all', 'last', 'bias', 'y0', 'g'}
    assert any(c.identity for c in cs) and any(not all(c.bias) for c in cs) and any(c.acts[-1] is not None for c in cs)
    for c in cs:                                               # a decreasing grid steps backwards; the non-uniform ones are non-uniform
        g = np.asarray(GC.GRIDS[c.grid])
        if c.grid.startswith('dec'):
            assert g[1] < g[0]
        if len(g) == 9:
            assert np.abs(g - (g[0] + (g[1] - g[0]) * np.arange(9)))[2:].min() > 0.1 * abs(g[1] - g[0])


def test_softplus_cases_reach_both_sides_of_the_threshold():
    for name in ('w127', 'f32_heun'):
        case = GC.BY_NAME[name]
        g = GC.make_g(case, dtype=F64)
        zs = []
        g[0].register_forward_hook(lambda m, i, o: zs.append(o.detach()))
        s = GC.solver_of(case, GC.make_f(case), g)
        with torch.no_grad():
            s._eager(N.HYPER_TRAJECTORY, torch.tensor(GC.grid_of(case)), torch.tensor(GC.y0_of(case)))
        z = torch.cat([v.reshape(-1) for v in zs])
        assert (z > 20.5).sum() >= 10 and ((z > -30) & (z < 19.5)).sum() >= 10 and (z < -30).sum() >= 10


# ---- the box ----------------------------------------------------------------------------------------------------------------------------
def _net(widths, act=nn.Tanh, dtype=F64):
    mods = []
    for i in range(len(widths) - 1):
        mods.append(nn.Linear(widths[i], widths[i + 1]))
        if i < len(widths) - 2:
            mods.append(act(widths[i + 1]) if act is nn.PReLU else act())
    return nn.Sequential(*mods).to(dtype)


class _Wrapped(nn.Module):
    def __init__(self, net):
        super(_Wrapped, self).__init__()
        self.net = net

    def forward(self, x):
        return self.net(x)


class _TrainableF(nn.Module):
    def __init__(self):
        super(_TrainableF, self).__init__()
        self.a = nn.Parameter(torch.tensor(0.7, dtype=F64))

    def forward(self, t, y):
        return torch.stack([y[..., 1], -self.a * y[..., 0]], dim=-1)


def test_the_box_function_gives_every_limit_its_reason():
    t = torch.tensor(GC.MAIN[:3], dtype=F64)
    y2, y3 = torch.randn(5, 2, dtype=F64), torch.randn(5, 3, dtype=F64)
    g2, g3 = _net([5, 17, 2]), _net([7, 17, 3])
    TRAJ, GRES = N.HYPER_TRAJECTORY, N.HYPER_G_RESIDUALS
    ok = [(R.Lorenz(), g3, TRAJ, t, y3), (R.LotkaVolterra(), g2, TRAJ, t, y2), (HR.lorenz_torch, g3, TRAJ, t, y3),
          (HR.forced_oscillator_torch, g2, TRAJ, t, y2.clone().requires_grad_(True)), (HR.lorenz_torch, g3, GRES, t, torch.randn(3, 4, 3, dtype=F64))]
    for args in ok:
        plan, why = H.describe_grad(*args)
        assert why is None and 'MI_ODE_DEFINE_HYPER_GRAD_PLUGIN' in plan['source'] and 'P = 0;' in plan['source'], why
        assert len(plan['params']) == 4 and plan['index'] == [(0, 1, None), (2, 3, None)]
    closes = torch.tensor(0.7, dtype=F64, requires_grad=True)
    bad = [
        ((_TrainableF(), g2, TRAJ, t, y2), 'trainable'),
        ((lambda t_, y: torch.stack([y[..., 1], -closes * y[..., 0]], dim=-1), g2, TRAJ, t, y2), 'trainable'),
        ((EC.ring(2), g2, TRAJ, t, y2), 'CustomRowLocal'),
        ((R.Linear(torch.tensor(EC.W2, dtype=F64)), g2, TRAJ, t, y2), 'Linear'),
        ((R.CubicLinear(torch.tensor(EC.W2C, dtype=F64)), g2, TRAJ, t, y2), 'CubicLinear'),
        ((R.Lorenz().reversed(), g3, TRAJ, t, y3), 'reversed'),
        ((R.Lorenz(), g3, TRAJ, t.clone().requires_grad_(True), y3), 't_span requires grad'),
        ((HR.lorenz_torch, g3, GRES, t, torch.randn(3, 4, 3, dtype=F64, requires_grad=True)), 'base trajectory requires grad'),
        ((R.Lorenz(), _net([7] + [128] * 5 + [3]), TRAJ, t, y3), 'size limit'),
        ((R.Lorenz(), _Wrapped(g3), TRAJ, t, y3), 'not an nn.Sequential'),
        ((R.Lorenz(), g3, N.HYPER_RESIDUAL, t, torch.randn(3, 4, 3, dtype=F64)), 'nothing to train'),
        ((R.Lorenz(), g3, TRAJ, t, y3.float()), 'parameters are not'),
        ((HR.lorenz_torch, g3, TRAJ, t, y3, False), 'lowering is off'),
        ((lambda t_, y: torch.roll(y, 1, 0), g3, TRAJ, t, y3), 'not lowered'),
    ]
    for args, word in bad:
        plan, why = H.describe_grad(*args)
        assert plan is None and word in why, (word, why)
    limit = H.describe_grad(R.Lorenz(), _net([7] + [128] * 5 + [3]), TRAJ, t, y3)[1]
    assert str(N.HYPER_GRAD_LDS_BYTES) in limit and limit.count('.') == 0          # one sentence, with the limit in it


def test_the_box_contains_the_nets_the_issue_names():
    t = torch.tensor(GC.MAIN[:3])
    for dtype in (torch.float64, torch.float32):
        y = torch.randn(4, 3, dtype=dtype)
        nets = {'notebook': _net([7, 64, 64, 64, 3], nn.PReLU, dtype), 'softplus128': _net([7, 128, 128, 3], nn.Softplus, dtype),
                'four_of_64': _net([7, 64, 64, 64, 3], nn.Tanh, dtype), 'three_of_128': _net([7, 128, 128, 3], nn.Tanh, dtype),
                'four_of_128': _net([7, 128, 128, 128, 3], nn.Tanh, dtype)}
        for name, g in nets.items():
            plan, why = H.describe_grad(R.Lorenz(), g, N.HYPER_TRAJECTORY, t.to(dtype), y)
            assert why is None, (name, dtype, why)
            assert plan['tile_bytes'] == H.grad_tile_bytes(plan['g'], dtype) <= N.HYPER_GRAD_LDS_BYTES
    # the tile formula is the library's (hyper_grad_layout)
    lib = N.load()
    for widths, dtype in (([7, 64, 64, 64, 3], torch.float64), ([5, 17, 2], torch.float32), ([7, 128, 128, 128, 3], torch.float64)):
        g = _net(widths, nn.Tanh, dtype)
        tab, _ = H.describe_g(g, widths[-1])
        d = N.HyperGradDesc()
        d.dtype, d.dim, d.n_layers, d.grid = N.dtype_code(dtype), widths[-1], len(widths) - 1, 1
        for j, (lin, act, _m) in enumerate(tab['layers']):
            d.layers[j].in_, d.layers[j].out, d.layers[j].act = lin.in_features, lin.out_features, act
        assert lib.mi_ode_hyper_grad_tile_bytes(C.byref(d)) == H.grad_tile_bytes(tab, dtype)
        assert lib.mi_ode_hyper_grad_workspace_bytes(C.byref(d)) > 0


def test_option_values_and_default():
    assert H.FUSED_GRAD is False and H.GRAD_GRID == 0
    g = _net([7, 17, 3])
    for v in (False, 'auto', True):
        assert H.HyperHeun(R.Lorenz(), g, options={'grad': v}).last_backward_stats == {}
    with pytest.raises(ValueError):
        H.HyperHeun(R.Lorenz(), g, options={'grad': 'yes'})


# ---- the host step core -----------------------------------------------------------------------------------------------------------------
_DRIVER = """
#include "mi_ode_hyper_grad.h"
// g = Linear(2 D + 1, H) tanh Linear(H, D) in plain loops, torch's [out][in] layout, with its vjp
struct DenseG {
  int D, H;
  const double *W1, *b1, *W2, *b2;
  double *gW1, *gb1, *gW2, *gb2;
  double x[16], h[64];
  void eval(const double* y, const double* k, double dt, double* out) {
    const int in = 2 * D + 1;
    for (int d = 0; d < D; ++d) { x[d] = y[d]; x[D + d] = k[d]; }
    x[2 * D] = dt;
    for (int j = 0; j < H; ++j) { double s = b1[j]; for (int i = 0; i < in; ++i) s += W1[j * in + i] * x[i]; h[j] = tanh(s); }
    for (int d = 0; d < D; ++d) { double s = b2[d]; for (int j = 0; j < H; ++j) s += W2[d * H + j] * h[j]; out[d] = s; }
  }
  void vjp(const double* gbar, double* xy, double* xk) {
    const int in = 2 * D + 1;
    double hb[64], xb[16];
    for (int j = 0; j < H; ++j) hb[j] = 0.0;
    for (int d = 0; d < D; ++d) { gb2[d] += gbar[d]; for (int j = 0; j < H; ++j) { gW2[d * H + j] += gbar[d] * h[j]; hb[j] += gbar[d] * W2[d * H + j]; } }
    for (int i = 0; i < in; ++i) xb[i] = 0.0;
    for (int j = 0; j < H; ++j) {
      const double zb = hb[j] * (1.0 - h[j] * h[j]);
      gb1[j] += zb;
      for (int i = 0; i < in; ++i) { gW1[j * in + i] += zb * x[i]; xb[i] += zb * W1[j * in + i]; }
    }
    for (int d = 0; d < D; ++d) { xy[d] = xb[d]; xk[d] = xb[D + d]; }
  }
};
template <int METHOD>
static void sweep_(DenseG& g, int T, int B, const double* t, const double* ys, const double* G, double* gy, const double* ps, const double* cw) {
  constexpr int D = RhsUser<double>::D;
  RhsUser<double> f(ps, cw);
  const double dt = t[1] - t[0];
  for (int r = 0; r < B; ++r) {
    double lam[D], yb[D];
    for (int d = 0; d < D; ++d) lam[d] = G[((long long)(T - 1) * B + r) * D + d];
    for (int i = T - 2; i >= 0; --i) {
      mi::hyper_grad_step<double, METHOD, D>(f, g, t[i], dt, ys + ((long long)i * B + r) * D, lam, yb);
      for (int d = 0; d < D; ++d) lam[d] = yb[d] + G[((long long)i * B + r) * D + d];
    }
    for (int d = 0; d < D; ++d) gy[(long long)r * D + d] = lam[d];
  }
}
extern "C" int hyper_grad_sweep(int method, int H, int T, int B, const double* t, const double* ys, const double* G, double* gy, const double* W1,
                                const double* b1, const double* W2, const double* b2, double* gW1, double* gb1, double* gW2, double* gb2,
                                const double* ps, const double* cw) {
  DenseG g{RhsUser<double>::D, H, W1, b1, W2, b2, gW1, gb1, gW2, gb2, {}, {}};
  if (method == mi::kHgEuler) sweep_<mi::kHgEuler>(g, T, B, t, ys, G, gy, ps, cw);
  else if (method == mi::kHgMidpoint) sweep_<mi::kHgMidpoint>(g, T, B, t, ys, G, gy, ps, cw);
  else if (method == mi::kHgHeun) sweep_<mi::kHgHeun>(g, T, B, t, ys, G, gy, ps, cw);
  else return -1;
  return 0;
}
"""
_LIBS = {}


def _compile(src, tag):
    d = tempfile.mkdtemp(prefix='hyper_grad_host_')
    cpp, so = os.path.join(d, tag + '.cpp'), os.path.join(d, tag + '.so')
    with open(cpp, 'w') as fh:
        fh.write(src)
    res = subprocess.run(['g++', '-O1', '-ffp-contract=off', '-std=c++17', '-shared', '-fPIC', '-I', N.CSRC, cpp, '-o', so], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return C.CDLL(so)


def _pool(tr):
    lay = L.Layout(tr)
    pool = np.zeros(max(lay.size, 1))
    for idx, off in enumerate(lay.tensor_off):
        x = tr.tensors[idx]['t'].detach()
        pool[off:off + x.numel()] = x.reshape(-1).double().cpu().numpy()
    pool[lay.extra_off:lay.extra_off + max(len(tr.scalars) - 8, 0)] = np.asarray(tr.scalars[8:])
    ps = (C.c_double * 8)(*(list(tr.scalars[:8]) + [0.0] * (8 - len(tr.scalars[:8]))))
    return pool, ps


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


_HOST_F = {'timed3': (GC.time_dependent_torch, 3), 'forced': (HR.forced_oscillator_torch, 2), 'lorenz': (HR.lorenz_torch, 3)}
_HOST_GRIDS = {'t2': (0.3, 0.55), 't5': GC.MAIN[:5], 't5_decreasing': GC.GRIDS['dec9'][:5], 't5_fine': GC.FINE[:5]}


@pytest.mark.parametrize('method', ['euler', 'midpoint', 'heun'])
@pytest.mark.parametrize('system,grid', [('timed3', 't5'), ('timed3', 't5_decreasing'), ('forced', 't2'), ('forced', 't5_decreasing'), ('lorenz', 't5_fine')])
def test_host_step_core_against_autograd(method, system, grid):
    """hyper_grad_step (the template the kernel instantiates) with a plain-loop g, g++: every gradient at the float64 bound.  A wrong dt / 2,
    dt^3 or a dropped dt * ybar2 shows here, without a GPU."""
    f, D = _HOST_F[system]
    Hd, B = 11, 3
    tr = L.trace(f, torch.zeros(2, D, dtype=F64))
    if system not in _LIBS:
        _LIBS[system] = _compile(L.host_vjp_source(tr) + _DRIVER, system)
    lib = _LIBS[system]
    gen = torch.Generator().manual_seed(5)
    g = nn.Sequential(nn.Linear(2 * D + 1, Hd), nn.Tanh(), nn.Linear(Hd, D)).double()
    cls = {'euler': H.HyperEuler, 'midpoint': H.HyperMidpoint, 'heun': H.HyperHeun}[method]
    t = torch.tensor(_HOST_GRIDS[grid], dtype=F64)
    y0 = (torch.tensor([1., 0.5, 0.8][:D], dtype=F64) + 0.3 * torch.randn(B, D, generator=gen, dtype=F64)).requires_grad_(True)
    G = torch.randn(len(t), B, D, generator=gen, dtype=F64)
    out = cls(f, g)._eager(N.HYPER_TRAJECTORY, t, y0)
    (out * G).sum().backward()
    ref = [y0.grad] + [p.grad for p in g.parameters()]
    assert all(float(r.abs().max()) > 0 for r in ref)
    pool, ps = _pool(tr)
    W1, b1, W2, b2 = (np.ascontiguousarray(p.detach().numpy()) for p in g.parameters())
    got = [np.zeros((B, D))] + [np.zeros_like(a) for a in (W1, b1, W2, b2)]
    ys, Gn, tt = np.ascontiguousarray(out.detach().numpy()), np.ascontiguousarray(G.numpy()), np.ascontiguousarray(t.numpy())
    rc = lib.hyper_grad_sweep({'euler': 0, 'midpoint': 1, 'heun': 2}[method], Hd, len(tt), B, _ptr(tt), _ptr(ys), _ptr(Gn), _ptr(got[0]), _ptr(W1), _ptr(b1),
                              _ptr(W2), _ptr(b2), _ptr(got[1]), _ptr(got[2]), _ptr(got[3]), _ptr(got[4]), ps, _ptr(pool))
    assert rc == 0
    for a, r in zip(got, ref):
        dev = float(np.abs(a - r.numpy()).max() / r.abs().max())
        assert dev <= GC.F64_BOUND, (method, system, grid, dev)


# ---- sources, ABI -----------------------------------------------------------------------------------------------------------------------
def test_generated_source_cross_compiles_for_gfx950():
    srcs = H.hyper_grad_sources(GC.time_dependent_torch, torch.zeros(2, 3, dtype=torch.float32))
    assert len(srcs) == 1 and 'static constexpr int P = 0;' in srcs[0] and '#include "mi_ode_hyper_grad_plugin.h"' in srcs[0]
    assert 'MI_ODE_PLUGIN_F32' in srcs[0] and 'mi_ode_discrete_plugin.h' not in srcs[0]
    path = PB.build(srcs[0])                             # hipcc --offload-arch=gfx950, as build() does (a cache hit after build())
    lib = C.CDLL(path)
    assert hasattr(lib, 'mi_ode_hyper_grad_plugin_get')
    all_ = GC.sources()
    assert len(all_) == len(set(all_)) and all('MI_ODE_DEFINE_HYPER_GRAD_PLUGIN(' in s or 'MI_ODE_DEFINE_HYPER_PLUGIN(' in s for s in all_)
    assert sum('MI_ODE_DEFINE_HYPER_GRAD_PLUGIN(' in s for s in all_) >= 8          # five systems, both dtypes where a case uses them
    assert H.hyper_grad_sources(EC.ring(2), torch.zeros(2, 2, dtype=F64)) == []
    # the forward's translation units and headers are untouched by the new plugin kind
    assert 'mi_ode_hyper_grad' not in open(os.path.join(N.CSRC, 'mi_ode_hyper_plugin.h')).read()
    assert 'mi_ode_hyper_grad' not in open(os.path.join(N.CSRC, 'mi_ode_hyper.h')).read()


def test_abi_is_13_and_the_entry_point_is_exported():
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    assert '#define MI_ODE_ABI_VERSION 13' in header and 'int mi_ode_hyper_grad_run(const mi_ode_hyper_grad* desc, void* stream);' in header
    assert N.ABI_VERSION == 13
    lib = N.load()
    assert lib.mi_ode_abi_version() == 13
    assert hasattr(lib, 'mi_ode_hyper_grad_run') and lib.mi_ode_hyper_grad_sizeof() == C.sizeof(N.HyperGradDesc)
    assert C.sizeof(N.HyperDesc) == C.sizeof(N.HyperGradDesc) - 8 * 2 - 3 * 8 * N.HYPER_MAX_LAYERS      # struct mi_ode_hyper stays as it is
    assert N.HYPER_GRAD_MAX_GRID == 256 and '#define MI_ODE_HYPER_GRAD_MAX_GRID 256' in header
