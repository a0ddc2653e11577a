"""CPU tests of the opt-in float64 fused mlp sweep of tfdiffeq_amd.discrete (csrc/mi_ode_discrete64.h): the C ABI (additive, version 13),
the refusals of mi_ode_discrete64_create, the `mlp64` switch and the routes that must not have moved.  No GPU needed."""
import ctypes as C
import os

import pytest
import torch

from tfdiffeq_amd import _native as N
from tfdiffeq_amd import adjoint as A
from tfdiffeq_amd import discrete as D
from tfdiffeq_amd import models, odeint_discrete

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mi_ode_discrete64_create', 'mi_ode_discrete64_destroy', 'mi_ode_discrete64_num_params', 'mi_ode_discrete64_sweep',
         'mi_ode_discrete64_profile')


def test_header_declares_the_five_symbols_and_abi_13():
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    for name in NAMES:
        assert name + '(' in header, name
    assert 'typedef struct mi_ode_discrete64* mi_ode_discrete64_handle;' in header
    assert '#define MI_ODE_ABI_VERSION 13' in header and N.ABI_VERSION == 13
    # the descriptor is the float32 sweep's: no new struct, no new mi_ode_sizeof index
    assert 'mi_ode_discrete64_create(const mi_ode_discrete_desc* desc, int32_t time_dependent' in header


def test_library_exports_the_five_symbols_with_the_bound_signatures():
    lib = N.load()                                           # (binds every prototype: a missing export raises here)
    assert lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_sizeof(9) == C.sizeof(N.DiscreteDesc)
    for name in NAMES:
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.mi_ode_discrete64_create.argtypes == [C.POINTER(N.DiscreteDesc), C.c_int32, C.POINTER(C.c_void_p)]
    assert lib.mi_ode_discrete64_sweep.argtypes == lib.mi_ode_discrete_sweep.argtypes
    assert lib.mi_ode_discrete64_num_params.restype is C.c_int64
    assert lib.mi_ode_discrete64_profile.argtypes == [C.c_void_p, C.POINTER(C.c_double)]
    assert lib.mi_ode_discrete64_num_params(None) == -1 and lib.mi_ode_discrete64_destroy(None) == 0
    assert lib.mi_ode_discrete64_profile(None, None) == N.E_INVALID


def _desc(dim=8, hidden=16, rows=3, n_points=5):
    d = N.DiscreteDesc()
    d.batch, d.dim, d.hidden, d.n_points = 40, dim, hidden, n_points
    d.tableau.n_stages = rows                                # rows + 1 stages
    return d


@pytest.mark.parametrize('kw,td,text', (
    (dict(dim=65), 0, 'dim <= 64'),
    (dict(hidden=129), 0, 'hidden <= 128'),
    (dict(rows=4), 0, 'at most 4 stages'),
    (dict(n_points=1), 0, 'n_points'),
    (dict(n_points=1026), 0, 'n_points <= 1025'),
    (dict(), 2, 'time_dependent must be 0 or 1'),
))
def test_create_refuses_what_is_outside_the_box(kw, td, text):
    lib = N.load()
    h = C.c_void_p()
    d = _desc(**kw)
    assert lib.mi_ode_discrete64_create(C.byref(d), td, C.byref(h)) == N.E_INVALID and not h.value
    assert text in N.last_error(), N.last_error()
    assert lib.mi_ode_discrete64_create(None, 0, C.byref(h)) == N.E_INVALID


def test_switch_defaults_to_off_and_rejects_other_values():
    assert D.MLP64 is False
    func = models.ODEFunc(4, 8, non_linearity='tanh')
    with pytest.raises(ValueError, match="mlp64 must be False, True or 'auto', not 'sometimes'"):
        odeint_discrete(func, torch.zeros(3, 4), torch.linspace(0., 1., 3), method='rk4', mlp64='sometimes')


class _DeviceLike(object):
    """What _fused_plan asks of `like` before it looks at the network: a tensor that says it is on the device."""

    def __init__(self, dtype):
        self.is_cuda, self.dtype = True, dtype


def test_fused_plan_answers():
    func = models.ODEFunc(4, 8, non_linearity='tanh').double()
    params = tuple(func.parameters())
    host = torch.zeros(3, 5, 4, dtype=torch.float64)
    for switch in ('auto', True):
        assert D._fused_plan(func, params, 'rk4', True, host, switch) == (None, 'a host tensor')
    assert D._fused_plan(func, params, 'rk4', True, host) == (None, 'a host tensor')
    # with the switch off the float64 answer is the old string, verbatim - whatever else holds
    assert D._fused_plan(func, params, 'rk4', True, _DeviceLike(torch.float64)) == (None, 'dtype float64 (the fused sweep is float32)')
    assert D._fused_plan(func, params, 'rk4', True, _DeviceLike(torch.float64), False) == (None, 'dtype float64 (the fused sweep is float32)')
    assert D._fused_plan(func, params, 'rk4', True, _DeviceLike(torch.float16), 'auto') == (None, 'dtype float16 (the fused sweeps are float32 and float64)')
    assert D._fused_plan(func, params, 'rk4', False, host, 'auto') == (None, 'a tuple state')


def test_the_float64_engines_have_their_own_cache_and_are_released(monkeypatch):
    import tfdiffeq_amd

    class Fake(object):
        made = []

        def __init__(self, *key):
            self.key, self.closed = key, False
            Fake.made.append(self)

        def close(self):
            self.closed = True
    monkeypatch.setattr(D, '_FusedDiscreteEngine64', Fake)
    monkeypatch.setattr(D, '_ENGINES64', {})
    before = dict(D._ENGINES)
    first = D._cached_engine64(33, 3, 5, 'rk4', 5, 'cuda:0', 0, True)
    assert D._cached_engine64(33, 3, 5, 'rk4', 5, 'cuda:0', 0, True) is first
    for n in range(6, 10):
        D._cached_engine64(33, 3, 5, 'rk4', n, 'cuda:0', 0, True)
    assert len(D._ENGINES64) == 4 and first.closed and not any(e.closed for e in Fake.made[1:])        # the oldest was evicted
    for key in D._ENGINES64:                                 # shape first, the dtype in the key, the chunk last
        assert key[:3] == (33, 3, 5) and 'float64' in key and key[-1] == 0
    assert D._ENGINES == before                              # the float32 cache is another one
    tfdiffeq_amd.clear_engine_cache()
    assert not D._ENGINES64 and all(e.closed for e in Fake.made)


def _recording_fused_plan(monkeypatch):
    """_fused_plan stands aside and records the length of the trajectory it was asked to plan for; mlp64=True then raises with its reason."""
    seen = []

    def fused_plan(func, params, method, tensor_input, like, mlp64=False):
        seen.append(int(like.shape[0]))
        return None, 'recorded'
    monkeypatch.setattr(D, '_fused_plan', fused_plan)
    monkeypatch.setattr(N, 'require_gpu_tensor', lambda *a, **k: None)
    return seen


def test_the_float64_check_plans_for_the_points_of_t_on_the_default_grid(monkeypatch):
    seen = _recording_fused_plan(monkeypatch)
    func = models.ODEFunc(4, 8, non_linearity='tanh').double()
    y0 = torch.zeros(3, 4, dtype=torch.float64, requires_grad=True)
    with pytest.raises(ValueError, match='recorded'):
        odeint_discrete(func, y0, torch.linspace(0., 1., 3, dtype=torch.float64), method='rk4', mlp64=True)
    assert seen == [3]


@pytest.mark.parametrize('lower', (False, 'auto'))
def test_the_float64_check_plans_for_the_segment_the_backward_sweeps_on_a_grid_of_its_own(monkeypatch, lower):
    """t has 2 points, step_size 1 / 8 gives 8 grid steps: the backward sweeps one segment of 9 grid states, whatever other switch is
    on (models.ODEFunc is a callable the row planner refuses: it does not lower to a row-local program)."""
    seen = _recording_fused_plan(monkeypatch)
    func = models.ODEFunc(4, 8, non_linearity='tanh').double()
    y0 = torch.zeros(3, 4, dtype=torch.float64, requires_grad=True)
    assert D._row_plan(func, tuple(func.parameters()), 'rk4', y0.detach())[0] is None
    with pytest.raises(ValueError, match='recorded'):
        odeint_discrete(func, y0, torch.tensor([0., 1.], dtype=torch.float64), method='rk4', options={'step_size': 1 / 8}, own_grid=True,
                        mlp64=True, lower=lower)
    assert seen == [9]


_MLP_KEY = lambda n: (33, 3, 5, 'rk4', n, 'cuda:0', 0, True)                                  # noqa: E731
_ADJ_KEY = lambda n: (33, 3, 5, 1e-6, 1e-8, 0.9, 10.0, 0.2, n, 'cuda:0', True)                   # noqa: E731
CACHES = {                                                   # name: (module, engine class, cache, key of n, close_on_evict)
    '_cached_engine': (D, '_FusedDiscreteEngine', '_ENGINES', _MLP_KEY, True),
    '_cached_engine64': (D, '_FusedDiscreteEngine64', '_ENGINES64', _MLP_KEY, True),
    '_cached_linear_engine': (D, '_FusedLinearEngine', '_LINEAR_ENGINES', lambda n: (17, 6, True, 'heun', n, 'cuda:0', torch.float64), False),
    '_cached_linear_grid_engine': (D, '_FusedLinearGridEngine', '_LINEAR_ENGINES', lambda n: (17, 6, True, 'heun', n, 3, 'cuda:0', torch.float64),
                                   False),
    '_cached_adjoint_engine': (A, '_FusedAdjointEngine', '_ENGINES', _ADJ_KEY, True),
    '_cached_linear_adjoint_engine': (A, '_LinearAdjointEngine', '_LIN_ENGINES',
                                      lambda n: (17, 6, torch.float64, 1e-6, 1e-8, 0.9, 10.0, 0.2, n, 'cuda:0'), True),
}


@pytest.mark.parametrize('name', sorted(CACHES))
def test_the_cache_contract_of_every_engine(monkeypatch, name):
    """A hit returns the same object; the fifth key evicts the oldest; a create that raises evicts nothing; an evicted MLP or adjoint engine
    is closed, an evicted linear sweep engine is only dropped (a pending plan may still hold it)."""
    mod, engine, cache, key, closes = CACHES[name]

    class Fake(object):
        made, fail = [], False

        def __init__(self, *args):
            if Fake.fail:
                raise N.NativeError('no memory')
            self.args, self.closed = args, False
            Fake.made.append(self)

        def close(self):
            self.closed = True
    monkeypatch.setattr(mod, engine, Fake)                     # (the class is looked up when the cache creates)
    monkeypatch.setattr(mod, cache, {})
    cached = getattr(mod, name)
    first = cached(*key(5))
    assert cached(*key(5)) is first and len(Fake.made) == 1 and first.args == key(5)
    for n in (6, 7, 8):
        cached(*key(n))
    assert len(getattr(mod, cache)) == 4 and not first.closed
    Fake.fail = True
    before = dict(getattr(mod, cache))
    with pytest.raises(N.NativeError):
        cached(*key(9))
    assert getattr(mod, cache) == before and list(getattr(mod, cache)) == list(before) and not any(e.closed for e in Fake.made)
    Fake.fail = False
    fifth = cached(*key(9))
    held = list(getattr(mod, cache).values())
    assert len(held) == 4 and first not in held and held[-1] is fifth and held[:3] == Fake.made[1:4]
    assert first.closed is closes and not any(e.closed for e in Fake.made[1:])
