"""Host tests of the fused linear sweep's routing (tfdiffeq_amd.discrete._linear_plan, odeint_discrete(linear=...)) and of its C ABI.  No GPU:
every refusal is decided before an engine is created, and the autograd function runs end to end on host tensors with the forward solve
replaced by the restatement's (tests/discrete_restatement.py), as tests/test_discrete_lowered_host.py does."""
import ctypes as C
import gc
import os

import pytest
import torch

from tfdiffeq_amd import _native as N
from tfdiffeq_amd import discrete as D
from tfdiffeq_amd import models, odeint_discrete
from tests import discrete_restatement as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


def _host_route(monkeypatch):
    def host_odeint(f, y0, t, method=None, options=None):
        return DR.solve(f, y0, t, method)
    host_odeint.last_stats = {}
    monkeypatch.setattr(D, 'odeint', host_odeint)
    monkeypatch.setattr(N, 'require_gpu_tensor', lambda *a, **k: None)


class LinModule(torch.nn.Module):
    """torch.nn.Linear(d, d) as a right-hand side: the matrix is [out, in], the layout the tracer reports as 'Wt'."""

    def __init__(self, d):
        super(LinModule, self).__init__()
        self.lin = torch.nn.Linear(d, d).double()

    def forward(self, t, y):
        return self.lin(y)


def _cases():
    """name -> (func, params, y0, n_points, fragment of the reason)."""
    g = torch.Generator().manual_seed(0)
    W8 = (torch.randn(8, 8, generator=g, dtype=F64) / 3).requires_grad_(True)
    b8 = torch.randn(8, generator=g, dtype=F64).requires_grad_(True)
    frozen_b = torch.randn(8, generator=g, dtype=F64)
    extra = torch.ones(8, dtype=F64).requires_grad_(True)
    W3 = torch.randn(3, 3, generator=g, dtype=F64).requires_grad_(True)
    W200 = (torch.randn(200, 200, generator=g, dtype=F64) / 20).requires_grad_(True)
    y8, y3, y200 = torch.randn(12, 8, generator=g, dtype=F64), torch.randn(12, 3, generator=g, dtype=F64), torch.randn(4, 200, generator=g, dtype=F64)
    mod = models.LinearODEFunc(8, bias=True, dtype=F64)
    mod_frozen = models.LinearODEFunc(8, bias=True, dtype=F64)
    mod_frozen.bias.requires_grad_(False)
    mod32 = models.LinearODEFunc(8, bias=False, dtype=F32)
    mod200 = models.LinearODEFunc(200, bias=False, dtype=F64)
    return {
        'tuple': (mod, tuple(mod.parameters()), (y8, y8), 4, 'a tuple state'),
        'host_module': (mod, tuple(mod.parameters()), y8, 4, 'a host tensor'),
        'host_callable': ((lambda t, y: y @ W8 + b8), (W8, b8), y8, 4, 'a host tensor'),
        'host_nn_linear': (LinModule(8), None, y8, 4, 'a host tensor'),
        'dtype': (mod, tuple(mod.parameters()), y8.half(), 4, 'dtype float16'),
        'dim_module': (mod200, tuple(mod200.parameters()), y200, 4, 'dim 200 > 128'),
        'dim_callable': ((lambda t, y: y @ W200), (W200,), y200, 4, 'dim 200 > 128'),
        'steps': (mod, tuple(mod.parameters()), y8, 1026, 'more than 1024 steps'),
        'frozen': (mod_frozen, (mod_frozen.weight,), y8, 4, 'frozen or extra parameters'),
        'frozen_callable': ((lambda t, y: y @ W8 + frozen_b), (W8,), y8, 4, 'frozen or extra parameters'),
        'extra': ((lambda t, y: y @ W8), (W8, extra), y8, 4, 'frozen or extra parameters'),
        'derived_transpose': ((lambda t, y: y @ W8.t()), (W8,), y8, 4, 'derived (non-leaf)'),
        'derived_tanh': ((lambda t, y: y @ torch.tanh(W8)), (W8,), y8, 4, 'derived (non-leaf)'),
        'param_dtype': (mod32, tuple(mod32.parameters()), y8, 4, 'parameters in another dtype'),
        'not_linear': ((lambda t, y: torch.tanh(y @ W3)), (W3,), y3, 4, 'family, not to y @ W'),
    }


@pytest.mark.parametrize('name', sorted(_cases()))
def test_refusals_of_the_fused_linear_route_say_why(name):
    f, params, y0, n_points, fragment = _cases()[name]
    if params is None:
        params = tuple(f.parameters())
    like = torch.empty((n_points,) + (tuple(y0.shape) if isinstance(y0, torch.Tensor) else ()), device='meta')
    plan, why = D._linear_plan(f, params, 'rk4', y0, like)
    assert plan is None and fragment in why, why


def test_the_plan_reaches_the_engine_for_every_accepted_form_and_reports_a_failed_create(monkeypatch):
    """With the device test out of the way, the module and the three callable forms get as far as the engine - asked for with the key the
    cache is indexed by - and a creation failure becomes a reason."""
    asked = []

    def fake_engine(*key):
        asked.append(key)
        raise N.NativeError('no device here')
    monkeypatch.setattr(D, '_cached_linear_engine', fake_engine)
    monkeypatch.setattr(D, '_on_device', lambda x: True)
    g = torch.Generator().manual_seed(1)
    W = (torch.randn(8, 8, generator=g, dtype=F64) / 3).requires_grad_(True)
    b = torch.randn(8, generator=g, dtype=F64).requires_grad_(True)
    y0 = torch.randn(12, 8, generator=g, dtype=F64)
    lin = LinModule(8)
    mod = models.LinearODEFunc(8, bias=True, dtype=F64)
    forms = [(mod, tuple(mod.parameters()), True), ((lambda t, y: y @ W), (W,), False), ((lambda t, y: y @ W + b), (b, W), True),
             (lin, tuple(lin.parameters()), True)]
    for f, params, has_bias in forms:
        plan, why = D._linear_plan(f, params, 'huen', y0, n_points=5)
        assert plan is None and 'the fused engine could not be created (no device here)' in why, why
        assert asked[-1] == (12, 8, has_bias, 'heun', 5, 'cpu', F64), asked[-1]


def test_the_transposed_layout_of_nn_linear_is_returned_in_the_parameters_layout():
    """_LinearPlan.sweep hands the kernel the [in, out] copy of an [out, in] matrix and transposes the gradient back, in the slots of the
    call's parameter list."""
    class Engine(object):
        def sweep(self, W, b, t, ys, grad_ys):
            self.W, self.b = W, b
            return torch.zeros(3, 2), torch.arange(4.).reshape(2, 2), torch.tensor([7., 8.])
    weight = torch.tensor([[1., 2.], [3., 4.]], requires_grad=True)          # [out, in]
    bias = torch.tensor([5., 6.], requires_grad=True)
    eng = Engine()
    plan = D._LinearPlan(weight, bias, 'Wt', [1, 0], eng)
    g_y0, gp = plan.sweep([0., 1.], torch.zeros(2, 3, 2), torch.zeros(2, 3, 2), 2)
    assert torch.equal(eng.W, weight.detach().t()) and eng.W.is_contiguous() and torch.equal(eng.b, bias.detach())
    assert torch.equal(gp[1], torch.arange(4.).reshape(2, 2).t()) and torch.equal(gp[0], torch.tensor([7., 8.]))
    with torch.no_grad():
        weight.mul_(2.0)                                                       # an in-place step is seen by the next call: nothing is cached
    plan.sweep([0., 1.], torch.zeros(2, 3, 2), torch.zeros(2, 3, 2), 2)
    assert torch.equal(eng.W, torch.tensor([[2., 6.], [4., 8.]]))


def test_unset_and_false_leave_the_routes_as_they_are_auto_says_why_true_raises(monkeypatch):
    _host_route(monkeypatch)
    assert D.LINEAR is False
    torch.manual_seed(3)
    func = models.LinearODEFunc(6, bias=True, dtype=F64)
    with torch.no_grad():
        func.bias.copy_(torch.randn(6, dtype=F64))
    params = tuple(func.parameters())
    g = torch.Generator().manual_seed(4)
    y0 = torch.randn(5, 6, generator=g, dtype=F64)
    t = torch.linspace(0., 1., 4, dtype=F64)
    w = torch.randn(4, 5, 6, generator=g, dtype=F64)
    _, gy, gp = DR.gradients(func, params, y0, t, 'rk4', w)
    seen = []
    for kw in ({}, {'linear': False}, {'linear': 'auto'}):
        odeint_discrete.last_backward_stats = {}
        y = y0.clone().requires_grad_(True)
        got = torch.autograd.grad((odeint_discrete(func, y, t, method='rk4', **kw) * w).sum(), (y,) + params)
        seen.append(dict(odeint_discrete.last_backward_stats))
        for a, b in zip(got, gy + gp):
            assert DR.rel_max(a, b) <= DR.ceiling64(3, 'rk4')
    odeint_discrete.last_backward_stats = {}
    y = y0.clone().requires_grad_(True)
    sol, = D._OdeintDiscrete.apply(func, func, 'rk4', None, t, True, len(params), *params, y)
    torch.autograd.grad((sol * w).sum(), (y,) + params)
    today = dict(odeint_discrete.last_backward_stats)
    assert seen[0] == today and seen[1] == today and today['engine'] == 'generic sweep', (seen, today)
    assert list(seen[0]) == list(today)
    assert seen[2]['engine'] == 'generic sweep' and 'fused linear sweep: a host tensor' in seen[2]['why'], seen[2]
    assert set(seen[2]) == set(today)
    with pytest.raises(ValueError, match='a host tensor'):
        odeint_discrete(func, y0.clone().requires_grad_(True), t, method='rk4', linear=True)
    with pytest.raises(ValueError, match='linear must be'):
        odeint_discrete(func, y0, t, method='rk4', linear='yes')
    # the module default is what an unset keyword reads (models.ODEBlock passes none)
    monkeypatch.setattr(D, 'LINEAR', 'auto')
    odeint_discrete.last_backward_stats = {}
    y = y0.clone().requires_grad_(True)
    torch.autograd.grad((odeint_discrete(func, y, t, method='rk4') * w).sum(), (y,) + params)
    assert 'fused linear sweep: a host tensor' in odeint_discrete.last_backward_stats['why']


def test_auto_on_a_refused_callable_returns_the_restatements_gradients(monkeypatch):
    _host_route(monkeypatch)
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(6, 6, generator=g, dtype=F64) / 3).requires_grad_(True)
    y0 = torch.randn(5, 6, generator=g, dtype=F64)
    t = torch.linspace(0., 1., 4, dtype=F64) ** 1.7
    w = torch.randn(4, 5, 6, generator=g, dtype=F64)

    def f(t_, y):
        return y @ W.t()
    _, gy, gp = DR.gradients(f, (W,), y0, t, 'heun', w)
    y = y0.clone().requires_grad_(True)
    got = torch.autograd.grad((odeint_discrete(f, y, t, method='heun', linear='auto') * w).sum(), (y, W))
    st = odeint_discrete.last_backward_stats
    assert st['engine'] == 'generic sweep' and 'fused linear sweep: a derived (non-leaf)' in st['why'], st
    for a, b in zip(got, gy + gp):
        assert DR.rel_max(a, b) <= DR.ceiling64(3, 'heun')
    with pytest.raises(ValueError, match='derived'):
        odeint_discrete(f, y0.clone().requires_grad_(True), t, method='heun', linear=True)


class _FakeEngine(object):
    """Stands for _FusedLinearEngine: a handle that sweeps only while it is open and is closed by its destructor."""
    made, closed = [], []

    def __init__(self, *key):
        self.key, self.h, self.stats = key, object(), N.Stats()
        self.stats.n_launches = 1
        _FakeEngine.made.append(self)

    def close(self):
        if self.h is not None:
            _FakeEngine.closed.append(self.key[0])
        self.h = None

    def __del__(self):
        self.close()

    def sweep(self, W, b, t, ys, grad_ys):
        if self.h is None:
            raise N.NativeError('mi_ode_discrete_linear_sweep: null argument')
        return torch.zeros_like(ys[0]), torch.full_like(W, float(self.key[0])), None


def test_an_evicted_or_cleared_engine_stays_open_for_the_plans_that_hold_it(monkeypatch):
    """Five forwards of distinct shape before any backward: the cache keeps four engines, and the first call's plan still sweeps.  Nothing
    closes an engine a pending plan holds - neither eviction nor clear_engines(); the last holder's release does."""
    _host_route(monkeypatch)
    monkeypatch.setattr(D, '_FusedLinearEngine', _FakeEngine)
    monkeypatch.setattr(D, '_on_device', lambda x: True)
    monkeypatch.setattr(D, '_LINEAR_ENGINES', {})
    _FakeEngine.made, _FakeEngine.closed = [], []
    t = torch.linspace(0., 1., 3, dtype=F64)
    calls = []
    for batch in (3, 4, 5, 6, 7):
        func = models.LinearODEFunc(6, bias=False, dtype=F64)
        y = torch.randn(batch, 6, dtype=F64).requires_grad_(True)
        calls.append((func, y, odeint_discrete(func, y, t, method='rk4', linear='auto')))
    assert len(_FakeEngine.made) == 5 and len(D._LINEAR_ENGINES) == 4
    first = _FakeEngine.made[0]
    assert first.key[0] == 3 and first.key not in D._LINEAR_ENGINES and first.h is not None     # evicted, still open
    D.clear_engines()
    assert not D._LINEAR_ENGINES and all(e.h is not None for e in _FakeEngine.made)                # every plan is still pending
    for func, y, sol in calls:
        odeint_discrete.last_backward_stats = {}
        sol.sum().backward()
        st = odeint_discrete.last_backward_stats
        assert st['engine'] == 'fused linear sweep' and st['n_launches'] == 1, st
        assert torch.equal(func.weight.grad, torch.full((6, 6), float(y.shape[0]), dtype=F64))      # each call swept on its own engine
    # the graph of a call holds its plan; with the graphs gone the handles are destroyed
    assert _FakeEngine.closed == []
    _FakeEngine.made = []
    del calls, func, y, sol, first
    gc.collect()
    assert sorted(_FakeEngine.closed) == [3, 4, 5, 6, 7]


def test_clear_engines_empties_both_caches_and_closes_what_nobody_holds():
    class Engine(object):
        closed = False

        def close(self):
            self.closed = True

        def __del__(self):
            self.close()
    seen = []
    e = Engine()
    e.close = lambda: seen.append('closed')
    D._LINEAR_ENGINES[('probe',)] = e
    D._ENGINES[('probe',)] = m = Engine()
    del e
    D.clear_engines()
    assert seen == ['closed'] and m.closed and not D._LINEAR_ENGINES and not D._ENGINES


def test_tracing_for_the_linear_route_does_not_count_as_an_evaluation(monkeypatch):
    """Under 'auto' a module that is not a LinearODEFunc is traced (its forward runs on proxies): its nfe counter is left as it was."""
    func = models.ODEFunc(6, 8, non_linearity='tanh').double()
    func.nfe = 3
    plan, why = D._linear_plan(func, tuple(func.parameters()), 'rk4', torch.randn(5, 6, dtype=F64), n_points=3)
    assert plan is None and why and func.nfe == 3, (why, func.nfe)


def test_c_abi_of_the_linear_sweep():
    names = ('mi_ode_discrete_linear_create', 'mi_ode_discrete_linear_destroy', 'mi_ode_discrete_linear_sweep')
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    for name in names:
        assert name in N.EXPORTED_SYMBOLS and name + '(' in header
    assert 'mi_ode_discrete_linear_desc' in header and '#define MI_ODE_ABI_VERSION 13' in header and N.ABI_VERSION == 13
    lib = N.load()                                           # (binds every prototype: a missing export raises here)
    assert lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_sizeof(11) == C.sizeof(N.DiscreteLinearDesc)
    for name in names:
        assert hasattr(lib, name)
    from tfdiffeq_amd.solvers import _fill_tableau
    h = C.c_void_p()
    assert lib.mi_ode_discrete_linear_create(None, C.byref(h)) == N.E_INVALID

    def desc(dim=16, n_points=3, dtype=N.F64, method='rk4'):
        d = N.DiscreteLinearDesc()
        d.dtype, d.dim, d.batch, d.has_bias, d.n_points = dtype, dim, 8, 0, n_points
        _fill_tableau(d.tableau, D.TABLEAUS[method], None)
        return d
    for bad in (desc(dim=129), desc(dim=0), desc(n_points=1), desc(n_points=1026), desc(dtype=77)):
        assert lib.mi_ode_discrete_linear_create(C.byref(bad), C.byref(h)) == N.E_INVALID and not h.value
    five = desc()
    five.tableau.n_stages = 4                                 # four rows: five stages
    assert lib.mi_ode_discrete_linear_create(C.byref(five), C.byref(h)) == N.E_INVALID and not h.value
    assert lib.mi_ode_discrete_linear_destroy(None) == 0
    assert lib.mi_ode_discrete_linear_sweep(None, None, None, None, None, None, None, None, None, None) == N.E_INVALID
