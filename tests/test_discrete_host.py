"""CPU tests of tfdiffeq_amd.discrete: the generic reverse sweep on host float64 tensors against autograd through the restatement of the
same discrete map (tests/discrete_restatement.py), the refusals, the ODEBlock keyword and the C ABI.  No GPU needed."""
import ctypes as C
import inspect
import os

import pytest
import torch

from tfdiffeq_amd import _native as N
from tfdiffeq_amd import discrete as D
from tfdiffeq_amd import models, odeint_discrete
from tests import discrete_restatement as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ('euler', 'midpoint', 'heun', 'rk4')


def _weights(shape, seed):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _check(func, params, y0, t, method, what):
    """generic_sweep from the restatement's own trajectory (the checkpoints) against autograd through the restatement, float64 ceiling."""
    tensor_input = isinstance(y0, torch.Tensor)
    ys0 = (y0,) if tensor_input else tuple(y0)
    n = t.shape[0]
    w = tuple(_weights((n,) + tuple(y.shape), 11 + i) for i, y in enumerate(ys0))
    sol, gy_ref, gp_ref = DR.gradients(func, params, y0, t, method, w[0] if tensor_input else w)
    tfunc = (lambda t_, y_: (func(t_, y_[0]),)) if tensor_input else (lambda t_, y_: tuple(func(t_, tuple(y_))))
    gy, gp = D.generic_sweep(tfunc, params, tuple(sol), t, w, method)
    ceil = DR.ceiling64(n - 1, method)
    for i, (a, b) in enumerate(zip(list(gy) + list(gp), gy_ref + gp_ref)):
        assert (a is None) == (b is None), '%s: tensor %d reached by one side only' % (what, i)
        if b is None:
            continue
        err = DR.rel_max(a, b)
        print('%s %s N=%d tensor %d: %.3e (ceiling %.3e)' % (what, method, n, i, err, ceil))
        assert err <= ceil, '%s %s N=%d tensor %d: max|got - ref| / max|ref| = %.3e above %.3e' % (what, method, n, i, err, ceil)


@pytest.mark.parametrize('n_points', (2, 5))
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('time_dependent', (False, True))
@pytest.mark.parametrize('act', ('tanh', 'softplus', 'relu'))
def test_generic_sweep_odefunc(act, time_dependent, method, n_points):
    torch.manual_seed(3)
    func = models.ODEFunc(6, 16, time_dependent=time_dependent, non_linearity=act).double()
    y0 = _weights((12, 6), 5)
    _check(func, tuple(func.parameters()), y0, torch.linspace(0., 1., n_points, dtype=torch.float64), method, 'ODEFunc %s td=%d' % (act, time_dependent))


@pytest.mark.parametrize('n_points', (2, 5))
@pytest.mark.parametrize('method', METHODS)
def test_generic_sweep_linear_odefunc(method, n_points):
    torch.manual_seed(4)
    func = models.LinearODEFunc(8, bias=True, dtype=torch.float64)
    with torch.no_grad():
        func.bias.add_(0.1 * _weights((8,), 6))
    _check(func, tuple(func.parameters()), _weights((10, 8), 7), torch.linspace(0., 1., n_points, dtype=torch.float64), method, 'LinearODEFunc')


@pytest.mark.parametrize('n_points', (2, 5))
@pytest.mark.parametrize('method', METHODS)
def test_generic_sweep_lambda_over_a_trainable_tensor(method, n_points):
    A = (0.5 * _weights((5, 5), 8)).requires_grad_(True)
    func = lambda t, y: torch.tanh(y @ A) * (1.0 + t)        # noqa: E731
    y0 = _weights((9, 5), 9)
    t = torch.linspace(0., 1., n_points, dtype=torch.float64)
    # the parameters of a plain callable are found as odeint finds them: the grad-requiring leaves of one evaluation
    params = D._params_of(func, y0, t)
    assert len(params) == 1 and params[0] is A
    _check(func, params, y0, t, method, 'lambda')


@pytest.mark.parametrize('n_points', (2, 5))
@pytest.mark.parametrize('method', METHODS)
def test_generic_sweep_tuple_state(method, n_points):
    torch.manual_seed(5)
    net = torch.nn.Linear(4, 3).double()

    def func(t, y):
        a, b = y
        return (torch.tanh(net(b)) - 0.3 * a, torch.sin(a).sum(-1, keepdim=True) * b * 0.2)
    y0 = (_weights((7, 3), 10), _weights((7, 4), 12))
    _check(func, tuple(net.parameters()), y0, torch.linspace(0., 1., n_points, dtype=torch.float64), method, 'tuple')


def test_out_of_scope_calls_raise_value_error():
    func = models.ODEFunc(4, 8, non_linearity='tanh')
    y0 = torch.zeros(3, 4)
    t = torch.linspace(0., 1., 3)
    for kw in (dict(method='dopri5'), dict(method='adaptive_heun'), dict(method='adams'), dict(method='fixed_adams'),
               dict(method='rk4', options={'step_size': 0.1}), dict(method='euler', options={'eps': 1e-3}),
               dict(method='rk4', options={'grid_constructor': lambda f, y, t_: t_})):
        with pytest.raises(ValueError, match='odeint_adjoint'):
            odeint_discrete(func, y0, t, **kw)
    with pytest.raises(ValueError, match='odeint_adjoint'):
        odeint_discrete(func, y0, t.clone().requires_grad_(True), method='rk4')
    for cls_kw in (dict(solver='dopri5'), dict(solver='adams'), dict()):
        with pytest.raises(ValueError):
            models.ODEBlock(func, gradient='discrete', **cls_kw)
    with pytest.raises(ValueError):
        models.ODENet(4, 8, 2, gradient='discrete', solver='dopri5')
    with pytest.raises(ValueError):
        models.ODEBlock(func, gradient='taped')


def test_gradient_keyword_defaults_to_adjoint_and_the_signature_is_otherwise_unchanged():
    sig = inspect.signature(models.ODEBlock.__init__)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ('odefunc', inspect.Parameter.empty), ('is_conv', False), ('tol', 1e-3), ('adjoint', False), ('solver', 'dopri5'), ('gradient', 'adjoint')]
    assert inspect.signature(models.ODENet.__init__).parameters['gradient'].default == 'adjoint'
    func = models.ODEFunc(4, 8, non_linearity='tanh')
    assert models.ODEBlock(func).gradient == 'adjoint'
    for solver in ('euler', 'midpoint', 'heun', 'huen', 'rk4'):
        assert models.ODEBlock(func, solver=solver, gradient='discrete').gradient == 'discrete'
    import tfdiffeq_amd
    assert tfdiffeq_amd.odeint_discrete is odeint_discrete and 'odeint_discrete' in tfdiffeq_amd.__all__


def test_last_backward_stats_after_a_backward(monkeypatch):
    """The autograd function end to end on host tensors (the forward solve, which has no host path, replaced by the restatement's):
    the gradients are the restatement's and last_backward_stats names the generic sweep, the step count and why the kernel was not used."""
    def host_odeint(f, y0, t, method=None, options=None):
        return DR.solve(f, y0, t, method)
    host_odeint.last_stats = {}
    monkeypatch.setattr(D, 'odeint', host_odeint)
    torch.manual_seed(7)
    func = models.ODEFunc(4, 8, non_linearity='tanh').double()
    params = tuple(func.parameters())
    t = torch.linspace(0., 1., 4, dtype=torch.float64)
    y0 = _weights((5, 4), 8).requires_grad_(True)
    w = _weights((4, 5, 4), 9)
    odeint_discrete.last_backward_stats = {}
    sol, = D._OdeintDiscrete.apply(func, func, 'rk4', None, t, True, len(params), *params, y0)
    got = torch.autograd.grad((sol * w).sum(), (y0,) + params)
    stats = odeint_discrete.last_backward_stats
    assert {'engine', 'n_steps', 'n_launches', 'why'} <= set(stats), stats
    assert stats['engine'] == 'generic sweep' and stats['n_steps'] == 3 and stats['n_launches'] is None and stats['why'] == 'a host tensor', stats
    _, gy, gp = DR.gradients(func, params, y0.detach(), t, 'rk4', w)
    for a, b in zip(got, gy + gp):
        assert DR.rel_max(a, b) <= DR.ceiling64(3, 'rk4')


def test_c_abi_symbols_and_struct_size():
    names = ('mi_ode_discrete_create', 'mi_ode_discrete_destroy', 'mi_ode_discrete_num_params', 'mi_ode_discrete_sweep')
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    for name in names:
        assert name in N.EXPORTED_SYMBOLS and name + '(' in header
    assert 'mi_ode_discrete_desc' in header and '#define MI_ODE_ABI_VERSION 13' in header
    assert N.ABI_VERSION == 13
    lib = N.load()                                           # (binds every prototype: a missing export raises here)
    assert lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_sizeof(9) == C.sizeof(N.DiscreteDesc)
    for name in names:
        assert hasattr(lib, name)
    # without a device the entry points refuse with an error code, they do not crash
    h = C.c_void_p()
    assert lib.mi_ode_discrete_create(None, C.byref(h)) == N.E_INVALID
    d = N.DiscreteDesc()
    d.batch, d.dim, d.hidden, d.n_points = 8, 200, 16, 3     # dim outside the tile box
    assert lib.mi_ode_discrete_create(C.byref(d), C.byref(h)) == N.E_INVALID and not h.value
    assert lib.mi_ode_discrete_num_params(None) == -1 and lib.mi_ode_discrete_destroy(None) == 0


def test_tableaus_are_the_solvers_own():
    from tfdiffeq_amd import fixed_grid
    assert D.TABLEAUS['euler'] is fixed_grid.Euler._fused_tableau and D.TABLEAUS['rk4'] is fixed_grid.RK4._fused_tableau
    assert D.TABLEAUS['huen'] is D.TABLEAUS['heun']
    for name, tab in D.TABLEAUS.items():
        assert len(tab.c_sol) == DR.STAGES[name] and abs(sum(tab.c_sol) - 1.0) < 1e-15


def test_clear_engine_cache_releases_the_sweep_engines():
    import tfdiffeq_amd

    class Engine(object):
        closed = False

        def close(self):
            self.closed = True
    eng = Engine()
    D._ENGINES[('stand-in',)] = eng
    tfdiffeq_amd.clear_engine_cache()
    assert eng.closed and not D._ENGINES
