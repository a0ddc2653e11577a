"""Host tests of odeint_discrete(own_grid=True): the grid plan against the restatement's own assignment, the gradients of the recompute-on-
the-grid route (one segment and three) against autograd through tests/discrete_grid_restatement.py, the refusals that stay, the ODEBlock
route and the C ABI of the own-grid linear kernel.  No GPU: the autograd function runs end to end on host tensors with the forward solve
replaced by the restatements', as tests/test_discrete_linear_host.py does."""
import ctypes as C
import os

import pytest
import torch

from tfdiffeq_amd import _native as N
from tfdiffeq_amd import discrete as D
from tfdiffeq_amd import models, odeint_discrete
from tests import discrete_grid_restatement as DGR
from tests import discrete_restatement as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
METHODS = ('euler', 'midpoint', 'heun', 'rk4')
# (t, step_size): a dyadic step - the hit at 0.25 is exact, two outputs share (0.25, 0.5], (0.5, 0.75] is empty; a clipped last step; a
# step larger than the span - one clipped step with every output interpolated inside it
PAIRS = {'dyadic': ([0., 0.25, 0.3, 0.4, 1.0], 0.25), 'clipped': ([0., 0.35, 0.7, 1.0], 0.3), 'one_step': ([0., 0.5, 1.0], 2.0)}


def _host_route(monkeypatch):
    def host_odeint(f, y0, t, method=None, options=None):
        step_size = (options or {}).get('step_size')
        return DR.solve(f, y0, t, method) if step_size is None else DGR.solve(f, y0, t, method, step_size)
    host_odeint.last_stats = {}
    monkeypatch.setattr(D, 'odeint', host_odeint)
    monkeypatch.setattr(N, 'require_gpu_tensor', lambda *a, **k: None)


@pytest.mark.parametrize('dtype', (F32, F64), ids=('float32', 'float64'))
@pytest.mark.parametrize('name', sorted(PAIRS))
def test_grid_plan_is_the_restatements_assignment(name, dtype):
    t, step = PAIRS[name]
    plan = D._grid_plan(torch.tensor(t, dtype=F64), step, dtype)
    grid, steps, weights = DGR.assignment(t, step, dtype)
    assert plan.grid.dtype == dtype and plan.out_w.dtype == dtype
    assert torch.equal(plan.grid, grid)
    assert list(plan.out_step) == steps and len(plan.out_step) == len(t)
    assert [float(w) for w in plan.out_w] == [float(torch.tensor(w, dtype=dtype)) for w in weights]
    # the grid is the solver's own constructor's, not a second implementation's
    from tfdiffeq_amd.solvers import FixedGridODESolver
    own = FixedGridODESolver._grid_constructor_from_step_size(None, step)(None, None, torch.tensor(t, dtype=F64).to(dtype))
    assert torch.equal(plan.grid, own)
    if name == 'dyadic':
        assert steps == [-1, 0, 1, 1, 3] and float(plan.out_w[1]) == 1.0 and float(plan.out_w[4]) == 1.0
        assert 0.0 < float(plan.out_w[2]) < float(plan.out_w[3]) < 1.0 and 2 not in steps
    elif name == 'clipped':
        assert grid.shape[0] == 5 and float(grid[-1]) == 1.0 and float(grid[-1] - grid[-2]) < 0.2      # the last step is clipped
        assert steps == [-1, 1, 2, 3] and float(plan.out_w[3]) == 1.0 and 0.0 < float(plan.out_w[1]) < 1.0
    else:
        assert grid.shape[0] == 2 and steps == [-1, 0, 0]
        assert [float(w) for w in plan.out_w] == [1.0, 0.5, 1.0]


# a hit on a grid point that becomes a segment boundary (0.375 = point 3 of 8 steps cut into 3 + 3 + 2), two outputs inside one step
T_SEG, STEP_SEG = [0., 0.375, 0.4, 0.45, 1.0], 0.125


def _problem(kind):
    g = torch.Generator().manual_seed(11)
    if kind == 'tensor':
        torch.manual_seed(12)
        func = models.ODEFunc(5, 7, time_dependent=True, non_linearity='tanh').double()
        return func, tuple(func.parameters()), torch.randn(6, 5, generator=g, dtype=F64)
    torch.manual_seed(13)
    net = torch.nn.Linear(4, 3).double()

    def func(t, y):
        a, b = y
        return torch.tanh(net(b)) * (1.0 + t), torch.sin(a) @ net.weight
    return func, tuple(net.parameters()), (torch.randn(5, 3, generator=g, dtype=F64), torch.randn(5, 4, generator=g, dtype=F64))


@pytest.mark.parametrize('segments', (1, 3))
@pytest.mark.parametrize('loss', ('every_output', 'last_output'))
@pytest.mark.parametrize('kind', ('tensor', 'tuple'))
@pytest.mark.parametrize('method', METHODS)
def test_recompute_route_returns_the_restatements_gradients(monkeypatch, method, kind, loss, segments):
    _host_route(monkeypatch)
    func, params, y0 = _problem(kind)
    ys0 = DR._tup(y0)
    t = torch.tensor(T_SEG, dtype=F64)
    g = torch.Generator().manual_seed(14)
    w = tuple(torch.randn((len(T_SEG),) + tuple(y.shape), generator=g, dtype=F64) for y in ys0)
    if loss == 'last_output':
        for w_ in w:
            w_[:-1] = 0.0
    _, gy, gp = DGR.gradients(func, params, y0, t, method, STEP_SEG, w[0] if kind == 'tensor' else w)
    n_grid = DGR.n_grid_steps(T_SEG, STEP_SEG, F64)
    assert n_grid == 8
    if segments == 3:                                        # room for 4 grid states and their gradients: segments of 3, 3 and 2 steps
        monkeypatch.setattr(D, 'GRID_BYTES', 8 * sum(y.numel() * y.element_size() for y in ys0))
    ysr = tuple(y.clone().requires_grad_(True) for y in ys0)
    odeint_discrete.last_backward_stats = {}
    sol = odeint_discrete(func, ysr[0] if kind == 'tensor' else ysr, t, method=method, options={'step_size': STEP_SEG}, own_grid=True)
    sol = DR._tup(sol)
    assert all(s.shape[0] == len(T_SEG) for s in sol)
    if loss == 'last_output':
        total = sum((w_[-1] * s[-1]).sum() for w_, s in zip(w, sol))
    else:
        total = sum((w_ * s).sum() for w_, s in zip(w, sol))
    got = torch.autograd.grad(total, ysr + params, allow_unused=True)
    st = odeint_discrete.last_backward_stats
    assert st['engine'] == 'generic sweep' and st['n_steps'] == n_grid, st
    assert st['own_grid'] == {'n_grid_steps': n_grid, 'n_segments': segments, 'recompute_launches': 2 * segments - 1}, st
    ceil = DR.ceiling64(n_grid, method)
    for i, (a, b) in enumerate(zip(got, gy + gp)):
        assert (a is None) == (b is None)
        if b is None:
            continue
        err = DR.rel_max(a, b)
        print('%s %s %s segments=%d tensor %d: %.3e (ceiling %.3e)' % (method, kind, loss, segments, i, err, ceil))
        assert err <= ceil, 'tensor %d: max|got - ref| / max|ref| = %.3e above %.3e' % (i, err, ceil)


@pytest.mark.parametrize('name', sorted(PAIRS))
def test_recompute_route_on_the_three_grids(monkeypatch, name):
    _host_route(monkeypatch)
    t_, step = PAIRS[name]
    func, params, y0 = _problem('tensor')
    t = torch.tensor(t_, dtype=F64)
    w = torch.randn((len(t_),) + tuple(y0.shape), generator=torch.Generator().manual_seed(15), dtype=F64)
    _, gy, gp = DGR.gradients(func, params, y0, t, 'rk4', step, w)
    y = y0.clone().requires_grad_(True)
    got = torch.autograd.grad((odeint_discrete(func, y, t, method='rk4', options={'step_size': step}, own_grid=True) * w).sum(), (y,) + params)
    n_grid = DGR.n_grid_steps(t_, step, F64)
    assert odeint_discrete.last_backward_stats['own_grid']['n_grid_steps'] == n_grid
    for a, b in zip(got, gy + gp):
        assert DR.rel_max(a, b) <= DR.ceiling64(n_grid, 'rk4')


def test_refusals_that_stay_and_the_default_without_step_size(monkeypatch):
    _host_route(monkeypatch)
    assert D.OWN_GRID is False and D.GRID_BYTES == 1 << 30 and D.GRID_KERNEL in (True, False)
    func = models.ODEFunc(4, 8, non_linearity='tanh')
    y0, t = torch.zeros(3, 4), torch.linspace(0., 1., 3)
    for kw in ({}, {'own_grid': False}):
        with pytest.raises(ValueError, match="options\\['step_size'\\] gives the solver a grid of its own.*odeint_adjoint"):
            odeint_discrete(func, y0, t, method='rk4', options={'step_size': 0.1}, **kw)
    with pytest.raises(ValueError, match='eps.*odeint_adjoint'):
        odeint_discrete(func, y0, t, method='rk4', options={'step_size': 0.1, 'eps': 1e-3}, own_grid=True)
    with pytest.raises(ValueError, match='grid_constructor.*odeint_adjoint'):
        odeint_discrete(func, y0, t, method='rk4', options={'grid_constructor': lambda f, y, t_: t_}, own_grid=True)
    with pytest.raises(ValueError, match='odeint_adjoint'):
        odeint_discrete(func, y0, t, method='dopri5', options={'step_size': 0.1}, own_grid=True)
    with pytest.raises(ValueError, match='requires grad'):
        odeint_discrete(func, y0, t.clone().requires_grad_(True), method='rk4', options={'step_size': 0.1}, own_grid=True)
    with pytest.raises(ValueError, match='own_grid must be'):
        odeint_discrete(func, y0, t, method='rk4', own_grid='yes')
    # a call without step_size is what it was: no new key in the stats
    y = torch.randn(3, 4).requires_grad_(True)
    odeint_discrete(func, y, t, method='rk4', own_grid=True).sum().backward()
    assert 'own_grid' not in odeint_discrete.last_backward_stats and odeint_discrete.last_backward_stats['n_steps'] == 2


def test_linear_auto_on_the_host_says_why_for_both_linear_sweeps(monkeypatch):
    _host_route(monkeypatch)
    func = models.LinearODEFunc(6, bias=True, dtype=F64)
    params = tuple(func.parameters())
    g = torch.Generator().manual_seed(16)
    y0 = torch.randn(5, 6, generator=g, dtype=F64)
    t_, step = PAIRS['clipped']
    t = torch.tensor(t_, dtype=F64)
    w = torch.randn(len(t_), 5, 6, generator=g, dtype=F64)
    _, gy, gp = DGR.gradients(func, params, y0, t, 'heun', step, w)
    for kernel in (True, False):
        monkeypatch.setattr(D, 'GRID_KERNEL', kernel)
        y = y0.clone().requires_grad_(True)
        got = torch.autograd.grad((odeint_discrete(func, y, t, method='heun', options={'step_size': step}, own_grid=True, linear='auto') * w).sum(),
                                  (y,) + params)
        st = odeint_discrete.last_backward_stats
        assert st['engine'] == 'generic sweep' and 'fused linear sweep: a host tensor' in st['why'], st
        assert ('fused linear sweep (own grid): ' + ('a host tensor' if kernel else 'discrete.GRID_KERNEL is False')) in st['why'], st
        for a, b in zip(got, gy + gp):
            assert DR.rel_max(a, b) <= DR.ceiling64(4, 'heun')
    with pytest.raises(ValueError, match='a host tensor'):
        odeint_discrete(func, y0.clone().requires_grad_(True), t, method='heun', options={'step_size': step}, own_grid=True, linear=True)


def test_the_own_grid_plan_asks_for_an_engine_keyed_by_steps_and_outputs(monkeypatch):
    asked = []

    def fake_engine(*key):
        asked.append(key)
        raise N.NativeError('no device here')
    monkeypatch.setattr(D, '_cached_linear_grid_engine', fake_engine)
    monkeypatch.setattr(D, '_on_device', lambda x: True)
    mod = models.LinearODEFunc(8, bias=True, dtype=F64)
    y0 = torch.randn(12, 8, dtype=F64)
    plan, why = D._linear_plan(mod, tuple(mod.parameters()), 'huen', y0, own_grid=(32, 2))
    assert plan is None and 'the fused engine could not be created (no device here)' in why, why
    assert asked == [(12, 8, True, 'heun', 32, 2, 'cpu', F64)]
    plan, why = D._linear_plan(mod, tuple(mod.parameters()), 'rk4', y0, own_grid=(1025, 2))
    assert plan is None and 'more than 1024 grid steps (1025)' in why and len(asked) == 1
    plan, why = D._linear_plan(mod, tuple(mod.parameters()), 'rk4', y0, own_grid=(1024, 1026))
    assert plan is None and 'more than 1025 outputs' in why and len(asked) == 1


def test_an_odeblock_with_a_step_size_trains_under_own_grid(monkeypatch):
    _host_route(monkeypatch)
    torch.manual_seed(17)
    func = models.ODEFunc(4, 8, non_linearity='tanh').double()
    block = models.ODEBlock(func, solver='rk4', gradient='discrete')
    monkeypatch.setattr(block, '_inference_func', lambda x: (func, None))       # (the fused descriptor has no host path)
    block.options = {'step_size': 1 / 16}
    x = torch.randn(6, 4, dtype=F64, generator=torch.Generator().manual_seed(18))
    with pytest.raises(ValueError, match='odeint_adjoint'):
        block(x)
    monkeypatch.setattr(D, 'OWN_GRID', True)
    params = tuple(func.parameters())
    _, gy, gp = DGR.gradients(func, params, x, torch.tensor([0., 1.], dtype=F64), 'rk4', 1 / 16,
                              torch.stack([torch.zeros_like(x), torch.ones_like(x)]))
    opt = torch.optim.SGD(func.parameters(), lr=0.1)
    before = [p.detach().clone() for p in params]
    opt.zero_grad()
    block(x).sum().backward()
    st = odeint_discrete.last_backward_stats
    assert st['n_steps'] == 16 and st['own_grid'] == {'n_grid_steps': 16, 'n_segments': 1, 'recompute_launches': 1}, st
    for p, b in zip(params, gp):
        assert DR.rel_max(p.grad, b) <= DR.ceiling64(16, 'rk4')
    opt.step()
    assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))


def _desc(dim=16, n_steps=4, n_out=3, dtype=N.F64, method='rk4'):
    from tfdiffeq_amd.solvers import _fill_tableau
    d = N.DiscreteLinearGridDesc()
    d.dtype, d.dim, d.batch, d.has_bias, d.n_steps, d.n_out = dtype, dim, 8, 0, n_steps, n_out
    _fill_tableau(d.tableau, D.TABLEAUS[method], None)
    return d


def test_c_abi_of_the_own_grid_linear_sweep():
    names = ('mi_ode_discrete_linear_grid_create', 'mi_ode_discrete_linear_grid_destroy', 'mi_ode_discrete_linear_grid_sweep',
             'mi_ode_discrete_linear_grid_validate', 'mi_ode_discrete_linear_grid_profile')
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    for name in names:
        assert name in N.EXPORTED_SYMBOLS and name + '(' in header
    assert 'mi_ode_discrete_linear_grid_desc' in header
    lib = N.load()
    assert lib.mi_ode_sizeof(12) == C.sizeof(N.DiscreteLinearGridDesc)
    assert lib.mi_ode_sizeof(11) == C.sizeof(N.DiscreteLinearDesc)                          # the default-grid descriptor is what it was
    assert [f[0] for f in N.DiscreteLinearDesc._fields_] == ['dtype', 'dim', 'batch', 'has_bias', 'n_points', 'tableau']
    for name in names:
        assert hasattr(lib, name)
    h = C.c_void_p()
    assert lib.mi_ode_discrete_linear_grid_create(None, C.byref(h)) == N.E_INVALID
    # every invalid descriptor is refused before the device is asked for: MI_ODE_E_INVALID (not MI_ODE_E_NODEVICE) on a host without one
    for bad in (_desc(dim=0), _desc(dim=129), _desc(n_steps=0), _desc(n_steps=1025), _desc(n_out=1), _desc(n_out=1026), _desc(dtype=77)):
        assert lib.mi_ode_discrete_linear_grid_create(C.byref(bad), C.byref(h)) == N.E_INVALID and not h.value
        assert lib.mi_ode_discrete_linear_grid_validate(C.byref(bad), None, None, None) == N.E_INVALID
    five = _desc()
    five.tableau.n_stages = 4
    assert lib.mi_ode_discrete_linear_grid_create(C.byref(five), C.byref(h)) == N.E_INVALID and not h.value
    good = _desc()
    grid = (C.c_double * 5)(0., 0.25, 0.5, 0.75, 1.)

    def check(steps, weights):
        return lib.mi_ode_discrete_linear_grid_validate(C.byref(good), grid, (C.c_int32 * 3)(*steps), (C.c_double * 3)(*weights))
    assert check([-1, 1, 3], [1., 0.5, 1.]) == 0
    assert check([-1, 3, 3], [1., 0., 1.]) == 0
    assert check([-1, 1, 4], [1., 0.5, 1.]) == N.E_INVALID                                 # outside [-1, n_steps)
    assert check([-1, -2, 3], [1., 0.5, 1.]) == N.E_INVALID
    assert check([0, 1, 3], [1., 0.5, 1.]) == N.E_INVALID                                  # output 0 is y0
    assert check([-1, 2, 1], [1., 0.5, 1.]) == N.E_INVALID                                 # decreasing
    assert check([-1, 1, 3], [1., 1.5, 1.]) == N.E_INVALID                                 # a weight outside [0, 1]
    assert check([-1, 1, 3], [1., -0.25, 1.]) == N.E_INVALID
    assert check([-1, 1, 3], [1., float('nan'), 1.]) == N.E_INVALID
    assert lib.mi_ode_discrete_linear_grid_destroy(None) == 0
    assert lib.mi_ode_discrete_linear_grid_sweep(None, None, None, None, None, None, None, None, None, None, None, None) == N.E_INVALID
    assert lib.mi_ode_discrete_linear_grid_profile(None, None, None) == N.E_INVALID
