"""GPU test of the dispatch (tfdiffeq_amd/dispatch.py): the route `odeint` reports (`last_stats['route']`), the engine `odeint.plan` names
and what actually ran agree - on the table of tests/test_host_logic.py (calls for which `plan` and the solvers used to disagree, and the same
calls on their fused routes) and on the five BASELINE right-hand sides at a batch that is certainly co-resident.  The test is about routes;
where the right-hand side has a numpy restatement (oracle.rhs_numpy through tests/rhs_util.py's names) the values are compared under the
bound the neighbouring tests use for that method in float64:
  dopri5          1e-9 of the solution's scale                  tests/test_gpu_tuple_fused.py::test_tuple_of_lorenz_states_runs_as_one_launch
  rk4             1e-12 absolute                                __graft_entry__.smoke, tests/test_gpu_tuple_fused.py
  tsit5           |diff| <= 1e-6 + 1e-5 |ref| (published tableau) tests/test_gpu_parity.py (assert_band, RTOL / ATOL)
  explicit_adams  1e-11 max(1, |ref|), oracle.adams_numpy        tests/test_gpu_multistep_fused.py::test_against_the_numpy_oracle
The two `step_size` rows are not compared: the numpy restatement mirrors the reference, whose step_size grid is dead code."""
import numpy as np
import pytest
import torch

from oracle import adams_numpy as OA
from oracle import ode_numpy as O
from oracle.rhs_numpy import make_rhs
from tests.rhs_util import device_rhs
from tests.test_host_logic import PLAN_ENGINE, ROUTE_CASES, route_state

pytestmark = pytest.mark.gpu

_LORENZ = {'sigma': 10., 'beta': 8. / 3., 'rho': 28.}
_LV = {'a': 1.5, 'b': 1., 'c': 3., 'd': 1.}
_SPIRAL = {'W': [[-0.1, 2.0], [-2.0, -0.1]]}
_S = np.random.RandomState(0).randn(128, 128)
_LINEAR = {'W': (-0.5 * np.eye(128) + 0.5 * (_S - _S.T) / np.sqrt(128.)).tolist()}


def _mlp():
    from tfdiffeq_amd import rhs
    torch.manual_seed(0)
    return rhs.from_sequential(torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.Tanh(), torch.nn.Linear(128, 128), torch.nn.Tanh(),
                                                   torch.nn.Linear(128, 64)))


BASELINE = [
    ('config 1: lotka-volterra rk4', lambda: device_rhs('lotka_volterra', _LV), [(1, 2)], torch.float64, 'rk4', None, 'fused'),
    ('config 2: spiral dopri5', lambda: device_rhs('cubic_linear', _SPIRAL), [(256, 2)], torch.float64, 'dopri5', None, 'fused'),
    ('config 3: lorenz tsit5', lambda: device_rhs('lorenz', _LORENZ), [(256, 3)], torch.float64, 'tsit5', None, 'fused'),
    ('config 4: linear dopri5', lambda: device_rhs('linear', _LINEAR), [(256, 128)], torch.float64, 'dopri5', None, 'fused'),
    ('config 5: mlp dopri5', _mlp, [(256, 64)], torch.float32, 'dopri5', None, 'fused'),
]


def _numpy_rhs(f):
    """The numpy restatement of a table row's right-hand side (oracle.rhs_numpy), where there is one."""
    from tfdiffeq_amd import rhs
    base = getattr(f, 'base', f)
    for cls, name, params in ((rhs.Lorenz, 'lorenz', _LORENZ), (rhs.LotkaVolterra, 'lotka_volterra', _LV), (rhs.CubicLinear, 'cubic_linear', _SPIRAL),
                              (rhs.Linear, 'linear', _LINEAR)):
        if type(base) is cls:
            g = make_rhs(name, params)
            return (lambda t, ys: tuple(g(t, y) for y in ys)) if getattr(f, 'per_component', False) else g
    return None


CASES = ROUTE_CASES + BASELINE


@pytest.mark.parametrize('name,make,shapes,dtype,method,options,kind', CASES, ids=[c[0] for c in CASES])
def test_route_plan_and_engine_agree(name, make, shapes, dtype, method, options, kind):
    from tfdiffeq_amd import odeint
    f, y0 = make(), route_state(shapes, dtype, 'cuda:0')
    t = torch.tensor([0., 0.02, 0.05], dtype=torch.float64)
    tol = dict(rtol=1e-7, atol=1e-9) if dtype == torch.float64 else dict(rtol=1e-4, atol=1e-6)
    sol = odeint(f, y0, t, method=method, options=options, **tol)
    st = dict(odeint.last_stats)
    p = odeint.plan(f, y0, t, method=method, options=options, **tol)
    print(name, 'route', st.get('route'), 'plan', p['engine'], p['launches'], 'engine', st.get('engine'), 'n_launches', st.get('n_launches'))
    assert st['route'] == kind
    assert p['engine'] == PLAN_ENGINE[kind], p
    if p['launches'].startswith('one per call'):
        assert st['n_launches'] == 1, st
    if kind == 'callable':
        assert st['engine'].startswith('device-controlled attempts'), st
    if kind == 'planes':
        assert st.get('engine', 'plane kernels').startswith('plane kernels') and st.get('n_launches') != 1, st
    g = _numpy_rhs(f)
    if g is None or dtype != torch.float64 or method not in ('dopri5', 'rk4', 'tsit5', 'explicit_adams') or 'step_size' in (options or {}):
        return
    tuple_state = isinstance(y0, tuple)
    y_np = tuple(y.cpu().numpy() for y in (y0 if tuple_state else (y0,)))
    if method == 'explicit_adams':
        ref = OA.FixedAdams(lambda t_, ys: (g(t_, ys[0]),), y_np, implicit=False, **tol).integrate(t.numpy())
    else:
        ref = O.odeint(g, y_np if tuple_state else y_np[0], t.numpy(), method=method, options={'tsit5_fixed': True} if method == 'tsit5' else None, **tol)
        ref = ref if tuple_state else (ref,)
    for got, rf in zip(sol if tuple_state else (sol,), ref):
        err, scale = np.abs(got.cpu().numpy() - rf), np.abs(rf).max()
        print(name, 'max|diff| %.3e, scale %.3e' % (err.max(), scale))
        if method == 'tsit5':
            assert (err <= 1e-6 + 1e-5 * np.abs(rf)).all()
        else:
            assert err.max() <= {'dopri5': 1e-9 * scale, 'rk4': 1e-12, 'explicit_adams': 1e-11 * max(1.0, scale)}[method]
