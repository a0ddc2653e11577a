"""Reverse mode over a row-local trace and the lowered route of `odeint_discrete`, as far as the CPU goes: the generated vjp and the
per-trajectory step template of the kernel (csrc/mi_ode_discrete_row.h) are compiled by g++ as host code and held to torch.autograd and
to the taped restatement tests/discrete_restatement.py."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discrete_lowered_cases as DC                       # noqa: E402
import discrete_restatement as DR                         # noqa: E402
import test_lower_trace as TLT                            # noqa: E402
from tfdiffeq_amd import _native as N                     # noqa: E402
from tfdiffeq_amd import discrete as D                    # noqa: E402
from tfdiffeq_amd import lower as L                       # noqa: E402
from tfdiffeq_amd import odeint_discrete                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _compile(src, tag, extra=()):
    d = tempfile.mkdtemp(prefix='discrete_lowered_')
    cpp, so = os.path.join(d, tag + '.cpp'), os.path.join(d, tag + '.so')
    with open(cpp, 'w') as fh:
        fh.write(src)
    res = subprocess.run(['g++', '-O1', '-ffp-contract=off', '-std=c++17', '-shared', '-fPIC'] + list(extra) + [cpp, '-o', so], capture_output=True, text=True)
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


def test_every_elementwise_function_has_a_vjp_rule_or_a_zero_entry():
    for fn in list(L._C_UN) + list(L._C_BIN) + ['where', 'powc']:
        assert fn in L._VJP_UN or fn in L._VJP_BIN or fn in L._VJP_ZERO or fn in ('where', 'powc'), fn
    assert not (set(L._VJP_ZERO) & (set(L._VJP_UN) | set(L._VJP_BIN)))
    for fn in ('floor', 'ceil', 'sign', 'gt', 'lt', 'ge', 'le', 'eq', 'ne'):
        assert fn in L._VJP_ZERO


# the operations of test_lower_trace.OPS with an operand made trainable where there is one: name -> make() -> (f, params)
def _trainable(name):
    W = (torch.arange(9, dtype=F64).reshape(3, 3) / 7 - 0.4).requires_grad_(True)
    v = torch.tensor([1., 2., 3.], dtype=F64, requires_grad=True)
    s = torch.tensor(0.6, dtype=F64, requires_grad=True)
    lin = torch.nn.Linear(3, 3).double()
    table = {
        'add_sub_mul_div': (lambda t, y: (y + v) * (y - 1.5) / (y * y + s), (v, s)),
        'rsub_rdiv': (lambda t, y: (s - y) + v / (y * y + 3), (s, v)),
        'pow_half': (lambda t, y: (y * y + s) ** 0.5 + (y * y + 1) ** -1 + (y * y + v) ** 1.5 + (y * y + 1) ** -0.5 + (y * y + 1) ** -2, (s, v)),
        'rpow': (lambda t, y: 2 ** (y * s) + (y * y + 1) ** v, (s, v)),
        'where_cmp': (lambda t, y: torch.where(y > 0, y * v, s * y), (v, s)),
        'clamp_max': (lambda t, y: torch.clamp(y * v, -0.5, 0.5) + torch.maximum(y, v) + torch.minimum(y, s), (v, s)),
        'time': (lambda t, y: y * torch.cos(t * s) + t ** 2 * v, (s, v)),
        'matmul_const': (lambda t, y: y @ W, (W,)),
        'linear_module': (lambda t, y: lin(y), tuple(lin.parameters())),
        'const_vector': (lambda t, y: y * v, (v,)),
        'sum_mean_keepdim': (lambda t, y: y - (y * v).sum(-1, keepdim=True) + y.mean(dim=-1, keepdim=True), (v,)),
        'norm': (lambda t, y: y / (y * v).norm(dim=-1, keepdim=True), (v,)),
        'index_stack': (lambda t, y: torch.stack([y[..., 1] * s, -y[..., 0], y[..., 2] * y[..., 0] * s], dim=-1), (s,)),
    }
    if name in table:
        return table[name]
    return TLT.OPS[name][0], ()


EXTRA_OPS = {
    'unary_rest': lambda t, y: (torch.tan(y * 0.3) + torch.sinh(y) * torch.cosh(y) + torch.asin(y * 0.2) + torch.acos(y * 0.2) + torch.atan(y)
                                + torch.log1p(y * y) + torch.expm1(y) + torch.exp2(y) + torch.log2(y * y + 1) + torch.log10(y * y + 1) + torch.erf(y)
                                + torch.log(y * y + 1) + torch.nn.functional.silu(y) + torch.rsqrt(y * y + 1) + torch.reciprocal(y * y + 2)
                                + torch.square(y) + torch.floor(y) + torch.ceil(y) + torch.sign(y) * y + torch.atan2(y, y * y + 1)),
    'matmul_traced': lambda t, y: (y.unsqueeze(-1) @ y.unsqueeze(-2)) @ torch.ones(3, dtype=F64) * 0.2,
    'matvec_left': lambda t, y, _W=(torch.arange(9, dtype=F64).reshape(3, 3) / 9).requires_grad_(True): (_W @ y.unsqueeze(-1)).squeeze(-1),
}


def _check_vjp(f, params, y0, tt=0.9, exact=False):
    tr = L.trace(f, y0)
    lib = _compile(L.host_vjp_source(tr), 'vjp')
    pool, ps = _pool(tr)
    plist, P = L.vjp_params(tr)
    assert all(any(tr.tensors[i]['t'] is p for p in params) for i, _o, _n in plist)
    rng = np.random.RandomState(1)
    rows = y0.reshape(-1, y0.shape[-1])
    for r in range(rows.shape[0]):
        kbar = rng.randn(rows.shape[1])
        y = rows[r:r + 1].clone().requires_grad_(True)
        out = f(torch.tensor(tt, dtype=F64), y)
        ref = torch.autograd.grad(out, (y,) + tuple(params), torch.tensor(kbar).reshape(out.shape), allow_unused=True)
        yin, ybar, tb = np.ascontiguousarray(rows[r].numpy()), np.zeros(rows.shape[1]), np.zeros(max(P, 1))
        lib.vjp_f64(C.c_double(tt), _ptr(yin), _ptr(kbar), _ptr(ybar), _ptr(tb), ps, _ptr(pool))
        refs = [np.zeros(rows.shape[1]) if ref[0] is None else ref[0].reshape(-1).numpy()]
        gots = [ybar]
        for i, off, n in plist:
            k = [j for j, p in enumerate(params) if p is tr.tensors[i]['t']][0]
            refs.append(np.zeros(n) if ref[1 + k] is None else ref[1 + k].reshape(-1).numpy())
            gots.append(tb[off:off + n])
        for got, want in zip(gots, refs):
            if exact:
                assert np.array_equal(got, want), (got, want)
            else:
                assert np.all(np.abs(got - want) <= 1e-12 * (1 + np.abs(want))), (got, want)


@pytest.mark.parametrize('name', sorted(TLT.OPS) + sorted(EXTRA_OPS))
def test_vjp_of_every_traced_operation(name):
    """ybar and the parameter contributions of the generated reverse code (g++) against torch.autograd.grad of the callable itself."""
    f, params = (EXTRA_OPS[name], ()) if name in EXTRA_OPS else _trainable(name)
    if name == 'matvec_left':
        params = (f.__defaults__[0],)
    y0 = torch.tensor(np.random.RandomState(0).randn(5, 3) * 0.7)          # (away from the kinks: no entry is 0, +-0.5 or an integer)
    _check_vjp(f, params, y0)


def test_vjp_conventions_at_ties():
    """torch.autograd's conventions where the derivative is a choice: relu'(0) = 0, abs'(0) = 0, clamp passes the gradient at its bounds,
    a maximum tie is split in halves - exactly."""
    y0 = torch.tensor([[0.0, -0.5, 0.5], [0.0, 0.5, -0.5]], dtype=F64)
    v = torch.tensor([0.0, -0.5, 0.5], dtype=F64, requires_grad=True)
    _check_vjp(lambda t, y: torch.relu(y) * 3, (), y0, exact=True)
    _check_vjp(lambda t, y: torch.abs(y) * 3, (), y0, exact=True)
    _check_vjp(lambda t, y: torch.clamp(y, -0.5, 0.5) * 3, (), y0, exact=True)
    _check_vjp(lambda t, y: torch.maximum(y, v) * 3 + torch.minimum(y, v), (v,), y0[:1], exact=True)


# ---- the whole sweep on the host: the kernel's step template (g++) around the generated functor -------------------------------------
def _tableau_arrays(method):
    tb = D.TABLEAUS[method]
    S = len(tb.alpha) + 1
    a, b, c = np.zeros((4, 4)), np.zeros(4), np.zeros(4)
    for i in range(1, S):
        c[i] = tb.alpha[i - 1]
        for j, v in enumerate(tb.beta[i - 1]):
            a[i, j] = v
    b[:S] = tb.c_sol[:S]
    return S, a, b, c


_SWEEP_LIBS = {}


_rel = DC.rel


def _host_sweep(name, method, t):
    f, params, y0 = DC.SYSTEMS[name]('cpu', F64)
    tr = L.trace(f, y0)
    if name not in _SWEEP_LIBS:
        _SWEEP_LIBS[name] = _compile(L.host_sweep_source(tr), 'sweep_' + name, extra=['-I', N.CSRC])
    lib = _SWEEP_LIBS[name]
    t = torch.tensor(t, dtype=F64)
    w = torch.randn((t.shape[0],) + tuple(y0.shape), generator=torch.Generator().manual_seed(7), dtype=F64)
    sol, gy, gp = DR.gradients(f, params, y0, t, method, w)
    dim = int(np.prod(tr.tail)) if tr.tail else 1
    ys = np.ascontiguousarray(sol[0].reshape(t.shape[0], -1, dim).numpy())
    gys = np.ascontiguousarray(w.reshape(t.shape[0], -1, dim).numpy())
    batch = ys.shape[1]
    plist, P = L.vjp_params(tr)
    gy0, gth = np.zeros((batch, dim)), np.zeros(max(P, 1))
    S, a, b, c = _tableau_arrays(method)
    pool, ps = _pool(tr)
    tt = np.ascontiguousarray(t.numpy())
    rc = lib.sweep_f64(S, _ptr(a), _ptr(b), _ptr(c), int(t.shape[0]), batch, _ptr(tt), _ptr(ys), _ptr(gys), _ptr(gy0), _ptr(gth), ps, _ptr(pool))
    assert rc == 0
    ceil = DR.ceiling64(t.shape[0] - 1, method)
    errs = [_rel(torch.tensor(gy0).reshape(y0.shape), gy[0])]
    for i, off, n in plist:
        k = [j for j, p in enumerate(params) if p is tr.tensors[i]['t']][0]
        errs.append(_rel(torch.tensor(gth[off:off + n]).reshape(params[k].shape), gp[k]))
    assert len(errs) == 1 + len(params)
    print(name, method, len(tt), ['%.2e' % e for e in errs], 'ceiling %.2e' % ceil)
    assert max(errs) <= ceil, (errs, ceil)


GRIDS = [('euler', 2), ('midpoint', 5), ('heun', 5), ('rk4', 5)]


@pytest.mark.parametrize('name', sorted(DC.SYSTEMS))
def test_host_sweep_matches_the_taped_restatement(name):
    """The reverse sweep of csrc/mi_ode_discrete_row.h's step template with the generated vjp, against autograd through the restatement."""
    T = DC.T_END[name]
    for method, n in GRIDS:
        _host_sweep(name, method, np.linspace(0., T, n))
    _host_sweep(name, 'rk4', np.array([0., .1, .35, .4, 1.]) * T)            # non-uniform
    _host_sweep(name, 'rk4', np.array([0., .1, .35, .4, 1.])[::-1].copy() * T)   # decreasing


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def _refusals():
    g = torch.Generator().manual_seed(0)
    W3 = torch.randn(3, 3, generator=g, dtype=F64).requires_grad_(True)
    W8 = (torch.randn(8, 8, generator=g, dtype=F64) / 3).requires_grad_(True)
    cb = torch.ones(40, 3, dtype=F64).mul(0.5).requires_grad_(True)
    c40 = torch.ones(40, dtype=F64).requires_grad_(True)
    net = torch.nn.Sequential(torch.nn.Linear(8, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(), torch.nn.Linear(32, 8)).double()
    y3, y8, y40 = torch.randn(40, 3, generator=g, dtype=F64), torch.randn(40, 8, generator=g, dtype=F64), torch.randn(6, 40, generator=g, dtype=F64)
    return {
        'derived': ((lambda t, y: torch.tanh(y @ W3.t())), (W3,), y3, 'derived (non-leaf)'),
        'batch_uniform': ((lambda t, y: -(cb * y)), (cb,), y3, 'batch axes'),
        'linear': ((lambda t, y: y @ W8), (W8,), y8, "'linear' family"),
        'mlp': ((lambda t, y: net(y)), tuple(net.parameters()), y8, "'mlp' family"),
        'coop': ((lambda t, y: torch.tanh(y) * c40), (c40,), y40, "'coop' family"),
        'tuple': ((lambda t, y: (-y[0], -y[1])), (), (y3, y3), 'tuple state'),
        'host': (DC.SYSTEMS['scalars']('cpu', F64)[0:1] + (None, None, 'a host tensor')),
    }


@pytest.mark.parametrize('name', ['derived', 'batch_uniform', 'linear', 'mlp', 'coop', 'tuple', 'host'])
def test_refusals_of_the_fused_row_local_route_say_why(name):
    f, params, y0, fragment = _refusals()[name]
    if name == 'host':
        f, params, y0 = DC.SYSTEMS['scalars']('cpu', F64)
    plan, why = D._row_plan(f, params, 'rk4', y0)
    assert plan is None and fragment in why, why


def _host_route(monkeypatch):
    def host_odeint(f, y0, t, method=None, options=None):
        return DR.solve(f, y0, t, method)
    host_odeint.last_stats = {}
    monkeypatch.setattr(D, 'odeint', host_odeint)
    monkeypatch.setattr(N, 'require_gpu_tensor', lambda *a, **k: None)


def test_the_default_and_lower_false_leave_the_routes_as_they_are(monkeypatch):
    """`lower` unset and lower=False: the stats of a backward are today's, key for key; 'auto' names why the row-local sweep was not used
    and still returns the gradients; True raises at the call."""
    _host_route(monkeypatch)
    assert D.LOWER is False and D.ROW_GRID == 0
    f, params, y0 = DC.SYSTEMS['scalars']('cpu', F64)
    t = torch.linspace(0., 1., 4, dtype=F64)
    w = torch.randn((4,) + tuple(y0.shape), generator=torch.Generator().manual_seed(3), dtype=F64)
    _, gy, gp = DR.gradients(f, params, y0, t, 'rk4', w)
    seen = []
    for kw in ({}, {'lower': False}, {'lower': 'auto'}):
        odeint_discrete.last_backward_stats = {}
        y = y0.clone().requires_grad_(True)
        got = torch.autograd.grad((odeint_discrete(f, y, t, method='rk4', **kw) * w).sum(), (y,) + params)
        seen.append(dict(odeint_discrete.last_backward_stats))
        for a, b in zip(got, gy + gp):
            assert DR.rel_max(a, b) <= DR.ceiling64(3, 'rk4')
    odeint_discrete.last_backward_stats = {}
    y = y0.clone().requires_grad_(True)
    sol, = D._OdeintDiscrete.apply(f, f, 'rk4', None, t, True, len(params), *params, y)
    torch.autograd.grad((sol * w).sum(), (y,) + params)
    today = dict(odeint_discrete.last_backward_stats)
    assert seen[0] == today and seen[1] == today and today['engine'] == 'generic sweep' and today['why'] == 'a host tensor', (seen, today)
    assert seen[2]['engine'] == 'generic sweep' and 'fused row-local sweep: a host tensor' in seen[2]['why'], seen[2]
    with pytest.raises(ValueError, match='a host tensor'):
        odeint_discrete(f, y0.clone().requires_grad_(True), t, method='rk4', lower=True)
    with pytest.raises(ValueError, match='lower must be'):
        odeint_discrete(f, y0, t, method='rk4', lower='yes')


def test_c_abi_of_the_row_sweep():
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    assert 'mi_ode_discrete_row_sweep' in N.EXPORTED_SYMBOLS and 'mi_ode_discrete_row_sweep(' in header and 'mi_ode_discrete_row_desc' in header
    assert '#define MI_ODE_ABI_VERSION 13' in header and N.ABI_VERSION == 13
    lib = N.load()
    assert lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_sizeof(10) == C.sizeof(N.DiscreteRowDesc) and lib.mi_ode_sizeof(9) == C.sizeof(N.DiscreteDesc)
    assert lib.mi_ode_discrete_row_sweep(None, None, None, None, None, None, None, None) == N.E_INVALID


def test_discrete_plugin_sources_are_stable_text_and_leave_the_row_local_plugins_alone():
    """The plugin cache is keyed by source text: two traces of the same callable give the same bytes; the discrete plugin includes its own
    header, and the row-local plugin's text does not change with the trainability of a tensor."""
    a, b = DC.discrete_sources('cpu'), DC.discrete_sources('cpu')
    assert a == b and len(a) >= 10
    for src in a:
        assert '#include "mi_ode_discrete_plugin.h"' in src and 'mi_ode_plugin.h' not in src and 'MI_ODE_DEFINE_DISCRETE_PLUGIN(mi::RhsUser)' in src
    f, params, y0 = DC.SYSTEMS['tanh8']('cpu', F64)
    before = L.sources_for(f, y0)
    for p in params:
        p.requires_grad_(False)
    assert L.sources_for(f, y0) == before
    assert L.vjp_params(L.trace(f, y0)) == ([], 0)
