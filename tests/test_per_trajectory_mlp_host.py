"""Per-trajectory step control for the ODEFunc network, host side (no GPU): what the route accepts and refuses - decided from the
descriptor, shapes, dtypes and options alone -, what `odeint.plan` reports for it, and the C entry point's declaration, export and
argument checks (include/mi_ode.h: mi_ode_integrate_rows_mlp; csrc/mi_ode_rows_mlp.h)."""
import ctypes as C
import os

import pytest
import torch

from tfdiffeq_amd import _native as N
from tfdiffeq_amd import dispatch as D
from tfdiffeq_amd import odeint, odeint_adjoint, rhs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
ON = {'per_trajectory': True}
T5 = torch.linspace(0., 1., 5, dtype=F64)


def mlp(dim=8, hidden=16, dtype=F32, activation='tanh', time_dependent=False):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype) / 3      # noqa: E731
    return rhs.MLP(r(dim + (1 if time_dependent else 0), hidden), r(hidden), r(hidden, hidden), r(hidden), r(hidden, dim), r(dim),
                   activation=activation, time_dependent=time_dependent)


def sequential(dim=8, hidden=16):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(dim, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, hidden), torch.nn.Tanh(),
                               torch.nn.Linear(hidden, dim))


# ---- acceptance: the route takes the call, only the device is missing ------------------------------------------------------------------------
def test_a_float32_mlp_is_accepted_and_only_the_device_is_missing():
    y = torch.ones(6, 8, dtype=F32)
    with pytest.raises(N.NativeError):                       # (a ValueError before this route existed)
        odeint(mlp(), y, T5, method='dopri5', options=ON)
    for method in ('tsit5', 'bosh3'):
        with pytest.raises(N.NativeError):
            odeint(mlp(activation='relu', time_dependent=True), y, T5, method=method, options=ON)


def test_from_sequential_and_a_lowered_sequential_are_accepted():
    y = torch.ones(6, 8, dtype=F32)
    seq = sequential()
    with pytest.raises(N.NativeError):
        odeint(rhs.from_sequential(seq), y, T5, method='dopri5', options=ON)
    with torch.no_grad(), pytest.raises(N.NativeError):      # a Python callable: traced, lowered to an 'mlp' program, routed to the same kernel
        odeint(lambda t, x: seq(x), y, T5, method='dopri5', options=ON)


def test_the_route():
    from tfdiffeq_amd.misc import _TupleFunc
    from tfdiffeq_amd.odeint import SOLVERS
    y = torch.ones(6, 8, dtype=F32)
    for method in ('dopri5', 'tsit5', 'bosh3'):
        route = SOLVERS[method](_TupleFunc(mlp()), (y,), rtol=1e-4, atol=1e-6, per_trajectory=True).route()
        assert route.kind == 'fused_rows_mlp' and route.why == D.ROWS_MLP_WHY and isinstance(route.rhs, rhs.MLP)
    assert SOLVERS['dopri5'](_TupleFunc(mlp()), (y,), rtol=1e-4, atol=1e-6).route().kind == 'fused'          # without the option: as it was
    assert SOLVERS['dopri5'](_TupleFunc(rhs.Lorenz()), (torch.ones(4, 3, dtype=F32),), rtol=1e-4, atol=1e-6, per_trajectory=True).route().kind == 'fused_rows'
    with pytest.raises(ValueError):
        SOLVERS['dopri5'](_TupleFunc(mlp()), (y,), rtol=1e-4, atol=1e-6, per_trajectory=True, rows_grid=-1)


# ---- refusals, each with its reason ---------------------------------------------------------------------------------------------------------------
def _refusals():
    y8, y8d = torch.ones(6, 8, dtype=F32), torch.ones(6, 8, dtype=F64)
    t2d = torch.linspace(0., 1., 5, dtype=F64).repeat(6, 1)
    return {
        'float64': (mlp(dtype=F64), y8d, T5, {}, {}, 'matrix-core or cooperative kernels (MLP', 'this state is float64'),
        'dim_65': (mlp(dim=65), torch.ones(6, 65, dtype=F32), T5, {}, {}, 'matrix-core or cooperative kernels (MLP, dim 65)', 'this network is 65 -> 16'),
        'hidden_129': (mlp(hidden=129), y8, T5, {}, {}, 'dim <= 64 and hidden <= 128', 'this network is 8 -> 129'),
        'dopri8': (mlp(), y8, T5, {'method': 'dopri8'}, {}, 'a 13-row tableau (dopri8)', 'dopri5, tsit5 and bosh3'),
        'adaptive_heun': (mlp(), y8, T5, {'method': 'adaptive_heun'}, {}, 'a 1-row tableau (adaptive_heun)', 'dopri5, tsit5 and bosh3'),
        't_2d': (mlp(), y8, t2d, {}, {}, 'per-row times, lengths or tolerances', 'k_rows_mlp reads one `t`'),
        't_lengths': (mlp(), y8, t2d, {}, {'t_lengths': torch.full((6,), 3, dtype=torch.int32)}, 'per-row times, lengths or tolerances', "options['t_lengths']"),
        'rtol_tensor': (mlp(), y8, T5, {'rtol': torch.full((6,), 1e-4, dtype=F64)}, {}, 'per-row times, lengths or tolerances', '`rtol` / `atol` tensors'),
        'y0_requires_grad': (mlp(), y8.clone().requires_grad_(True), T5, {}, {}, 'inputs that require grad', 'odeint_adjoint'),
        'tuple_state': (mlp(), (y8, y8), T5, {}, {}, 'a tuple state of several components', 'one [batch, dim] tensor'),
        'sharded': (mlp(), y8, T5, {}, {'process_group': object()}, 'a sharded run', 'shard the batch yourself'),
        'force_planes': (mlp(), y8, T5, {}, {'force_plane_kernels': True}, "options['force_plane_kernels']", 'shared control only'),
    }


@pytest.mark.parametrize('name', sorted(_refusals()))
def test_refusals_raise_value_error_with_the_reason(name):
    f, y0, t, kw, extra, first, second = _refusals()[name]
    kw = dict({'method': 'dopri5'}, **kw)
    with pytest.raises(ValueError) as e:
        odeint(f, y0, t, options=dict(ON, **extra), **kw)
    msg = str(e.value)
    assert "options['per_trajectory'] refused" in msg and first in msg and second in msg, msg
    plan = odeint.plan(f, y0, t, options=dict(ON, **extra), **kw)
    assert plan['engine'] == 'refused' and first in plan['why'], plan


def test_a_lowered_sequential_that_requires_grad_is_refused():
    seq, y = sequential(), torch.ones(6, 8, dtype=F32)
    with pytest.raises(ValueError) as e:
        odeint(lambda t, x: seq(x), y, T5, method='dopri5', options=ON)
    assert 'inputs that require grad' in str(e.value)


def test_odeint_adjoint_with_the_option_stays_refused_and_names_the_forward_route():
    y = torch.ones(6, 8, dtype=F32)
    seq = sequential()

    class F(torch.nn.Module):
        def __init__(self):
            super(F, self).__init__()
            self.net = seq

        def forward(self, t, x):
            return self.net(x)
    from tfdiffeq_amd import models
    for f in (F(), models.ODEFunc(8, 16, non_linearity='tanh')):
        with pytest.raises(ValueError) as e:
            odeint_adjoint(f, y, T5, method='dopri5', options=ON)
        msg = str(e.value)
        assert "options['per_trajectory'] refused" in msg and 'k_rows_mlp' in msg and 'no backward kernel' in msg, msg


# ---- odeint.plan ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim,hidden,method,S,geom', [(8, 16, 'dopri5', 6, '16, 16'), (20, 100, 'tsit5', 6, '64, 128'), (64, 16, 'bosh3', 3, '64, 16'),
                                                       (16, 128, 'dopri5', 6, '16, 128')])
def test_plan_reports_the_route_without_a_device(dim, hidden, method, S, geom):
    y = torch.ones(70, dim, dtype=F32)
    p = odeint.plan(mlp(dim, hidden, activation='relu'), y, T5, method=method, options=ON)
    assert p['engine'] == 'fused' and p['per_trajectory'] is True and p['launches'] == 'one per call' and p['why'] == D.ROWS_MLP_WHY, p
    assert p['kernel'].startswith('k_rows_mlp<%s, relu, %d, ..>' % (geom, S)), p
    assert p['state'] == '70 x %d float32' % dim and p['lower'] is None
    seq = sequential()
    with torch.no_grad():
        low = odeint.plan(lambda t, x: seq(x), torch.ones(5, 8, dtype=F32), T5, method='dopri5', options=ON)
    assert low['engine'] == 'fused' and low['kernel'].startswith('k_rows_mlp<16, 16, tanh, 6') and low['lower']['kind'] == 'mlp', low


# ---- header, exports, ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    assert 'int mi_ode_integrate_rows_mlp(mi_ode_handle h, const mi_ode_rows_mlp_desc* desc,' in header
    assert 'int64_t mi_ode_rows_mlp_sizeof(void);' in header and 'typedef struct mi_ode_rows_mlp_desc {' in header
    assert 'mi_ode_integrate_rows_mlp' in N.EXPORTED_SYMBOLS and 'mi_ode_rows_mlp_sizeof' in N.EXPORTED_SYMBOLS
    assert '#define MI_ODE_ABI_VERSION 13' in header and N.ABI_VERSION == 13
    lib = N.load()
    assert hasattr(lib, 'mi_ode_integrate_rows_mlp') and lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_sizeof(0) == C.sizeof(N.Desc) == 2360 and lib.mi_ode_sizeof(1) == C.sizeof(N.Stats) == 88
    assert lib.mi_ode_rows_mlp_sizeof() == C.sizeof(N.RowsMlpDesc) == 8
    assert [f[0] for f in N.RowsMlpDesc._fields_] == ['grid', 'reserved']


def test_null_arguments_are_invalid():
    lib = N.load()
    assert lib.mi_ode_integrate_rows_mlp(None, None, None, None, 0, None, None, None, None) == N.E_INVALID
    d = N.RowsMlpDesc()
    assert lib.mi_ode_integrate_rows_mlp(None, C.byref(d), None, None, 2, None, None, None, None) == N.E_INVALID
    assert 'bad argument' in N.last_error()
