"""Per-trajectory step control (options={'per_trajectory': True}, csrc/mi_ode_rows.h) as far as the CPU goes: the refusals, the C ABI, what
`odeint.plan` reports, and the per-row integration itself - csrc/mi_ode_rows_core.h compiled by g++ around the catalogue functors and
held, row by row, to the oracle's batch-1 solve (attempt and accept counts exactly)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_trajectory_cases as PC                          # noqa: E402
from oracle import ode_numpy as O                         # noqa: E402
from tfdiffeq_amd import _native as N                     # noqa: E402
from tfdiffeq_amd import odeint, rhs                      # noqa: E402
from tfdiffeq_amd.bosh3 import _BOGACKI_SHAMPINE_TABLEAU, BS_C_MID   # noqa: E402
from tfdiffeq_amd.dopri5 import _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
T5 = torch.linspace(0., 1., 5, dtype=F64)
ON = {'per_trajectory': True}


# ---- refusals: a ValueError with the reason, decided without a device (every state here is a host tensor) ---------------------------------
def _refusals():
    g = torch.Generator().manual_seed(0)
    y3, y8, y40 = torch.randn(6, 3, generator=g, dtype=F64), torch.randn(6, 8, generator=g, dtype=F64), torch.randn(6, 40, generator=g, dtype=F64)
    W8 = torch.randn(8, 8, generator=g, dtype=F64) / 3
    mlp = rhs.MLP(torch.randn(8, 16, dtype=F64), torch.zeros(16, dtype=F64), torch.randn(16, 16, dtype=F64), torch.zeros(16, dtype=F64),
                  torch.randn(16, 8, dtype=F64), torch.zeros(8, dtype=F64))
    coop = rhs.CustomCoop(40, "k = -y[i];", torch_fn=lambda t, y: -y)
    conv = rhs.Conv2dODE(torch.zeros(4, 2, 1, 1, dtype=F64), torch.zeros(4, dtype=F64), torch.zeros(4, 4, 3, 3, dtype=F64), torch.zeros(4, dtype=F64),
                         torch.zeros(2, 4, 1, 1, dtype=F64), torch.zeros(2, dtype=F64))
    lor = rhs.Lorenz()
    return {
        'euler': (lor, y3, 'euler', {}, 'a fixed-grid or Adams method'),
        'rk4': (lor, y3, 'rk4', {}, 'a fixed-grid or Adams method'),
        'adams': (lor, y3, 'adams', {}, 'a fixed-grid or Adams method'),
        'fixed_adams': (lor, y3, 'fixed_adams', {}, 'a fixed-grid or Adams method'),
        'tuple_state': ((lambda t, y: (-y[0], -y[1])), (y3, y3), 'dopri5', {}, 'a tuple state of several components'),
        'per_component': (rhs.PerComponent(lor), (y3, y3), 'dopri5', {}, 'rhs.PerComponent'),
        'linear': (rhs.Linear(W8), y8, 'dopri5', {}, 'matrix-core or cooperative kernels (Linear, dim 8)'),
        'mlp': (mlp, y8, 'dopri5', {}, 'matrix-core or cooperative kernels (MLP'),
        'custom_coop': (coop, y40, 'dopri5', {}, 'matrix-core or cooperative kernels (CustomCoop, dim 40)'),
        'conv2d': (conv, torch.zeros(2, 2, 6, 6, dtype=F64), 'dopri5', {}, 'matrix-core or cooperative kernels (Conv2dODE'),
        'lowered_40_elements': ((lambda t, y: torch.tanh(y) * 1.5), y40, 'dopri5', {}, "a lowered 'coop' program, dim 40"),
        'lowered_linear': ((lambda t, y: y @ W8), y8, 'dopri5', {}, "a lowered 'linear' program"),
        'tracer_refuses': ((lambda t, y: y * float(y.sum())), y3, 'dopri5', {}, 'the tracer refuses this callable'),
        'lower_false': ((lambda t, y: -y), y3, 'dopri5', {'lower': False}, "options['lower'] is False"),
        'sharded': (lor, y3, 'dopri5', {'process_group': object()}, 'a sharded run'),
        'y0_requires_grad': (lor, y3.clone().requires_grad_(True), 'dopri5', {}, 'odeint_adjoint without the option'),
        'closure_requires_grad': ((lambda t, y, _w=torch.ones(3, dtype=F64, requires_grad=True): -y * _w), y3, 'dopri5', {}, 'odeint_adjoint without the option'),
        'value_string': (lor, y3, 'dopri5', {'per_trajectory': 'yes'}, 'must be True or False'),
        'value_one': (lor, y3, 'dopri5', {'per_trajectory': 1}, 'must be True or False'),
    }


@pytest.mark.parametrize('name', sorted(_refusals()))
def test_refusals_raise_value_error_with_the_reason(name):
    f, y0, method, extra, fragment = _refusals()[name]
    with pytest.raises(ValueError) as e:
        odeint(f, y0, T5, method=method, options=dict(ON, **extra))
    assert fragment in str(e.value), str(e.value)
    if not name.startswith('value_'):
        assert "options['per_trajectory'] refused" in str(e.value)


def test_false_and_absent_are_the_same_call():
    """per_trajectory=False reaches the solver as if the key were absent: the same route, the same refusal of a host tensor."""
    from tfdiffeq_amd import dispatch as D
    from tfdiffeq_amd.odeint import SOLVERS
    from tfdiffeq_amd.misc import _TupleFunc
    y = torch.ones(4, 3, dtype=F64)
    a = SOLVERS['dopri5'](_TupleFunc(rhs.Lorenz()), (y,), rtol=1e-6, atol=1e-9)
    b = SOLVERS['dopri5'](_TupleFunc(rhs.Lorenz()), (y,), rtol=1e-6, atol=1e-9, per_trajectory=False)
    c = SOLVERS['dopri5'](_TupleFunc(rhs.Lorenz()), (y,), rtol=1e-6, atol=1e-9, per_trajectory=True)
    assert a.route().kind == b.route().kind == 'fused' and c.route().kind == 'fused_rows' and c.route().why == D.ROWS_WHY
    assert D.per_trajectory_option({'per_trajectory': False, 'x': 1}) == ({'x': 1}, False) and D.per_trajectory_option(None) == (None, False)
    with pytest.raises(N.NativeError):
        odeint(rhs.Lorenz(), y, T5, method='dopri5', options={'per_trajectory': False})
    with pytest.raises(N.NativeError):                       # accepted (no ValueError): it is the device that is missing
        odeint(rhs.Lorenz(), y, T5, method='dopri5', options=ON)
    with pytest.raises(N.NativeError):
        odeint(PC.time_callable, torch.ones(4, PC.TIME_DIM, dtype=F64), T5, method='dopri5', options=ON)


# ---- header, exports, ABI ----------------------------------------------------------------------------------------------------------------
def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    assert 'int mi_ode_integrate_rows(mi_ode_handle h,' in header and 'mi_ode_integrate_rows' in N.EXPORTED_SYMBOLS
    assert '#define MI_ODE_ABI_VERSION 13' in header and N.ABI_VERSION == 13
    lib = N.load()
    assert hasattr(lib, 'mi_ode_integrate_rows') and lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_sizeof(0) == C.sizeof(N.Desc) == 2360 and lib.mi_ode_sizeof(1) == C.sizeof(N.Stats) == 88
    plugin_h = open(os.path.join(N.CSRC, 'mi_ode_plugin.h')).read()
    assert '#define MI_ODE_PLUGIN_ABI 3' in plugin_h and 'rows' not in plugin_h
    assert lib.mi_ode_integrate_rows(None, None, None, None, 0, None, None, None, None) == N.E_INVALID


def test_rows_source_generates_a_translation_unit_of_its_own_kind():
    vdp = PC.van_der_pol()
    for dt in PC.DTYPES:
        src, base = vdp.rows_source(dt), vdp.source(dt)
        assert '#include "mi_ode_rows_plugin.h"' in src and 'MI_ODE_DEFINE_ROWS_PLUGIN(mi::RhsUser)' in src
        assert 'mi_ode_plugin.h"' not in src and 'MI_ODE_DEFINE_ROWLOCAL_PLUGIN' not in src
        assert '#include "mi_ode_plugin.h"' in base                 # (the row-local plugin's text - its cache key - is untouched)
    from tfdiffeq_amd import _plugin_build as PB
    roots = PB._source_roots(vdp.rows_source(F64))
    assert roots == ('mi_ode_rows_plugin.h',)
    hashed = [os.path.basename(p) for p in PB._plugin_headers(roots)]
    assert 'mi_ode_rows.h' in hashed and 'mi_ode_rows_core.h' in hashed and 'mi_ode_persist.h' in hashed
    assert 'mi_ode_rows.h' not in [os.path.basename(p) for p in PB._plugin_headers()]     # row-local plugins are not rebuilt for this feature
    with pytest.raises(ValueError):
        rhs.rows_source_of(rhs.CustomCoop(40, "k = -y[i];").source(F64))
    a, b = PC.rows_sources('cpu'), PC.rows_sources('cpu')
    assert a == b and len(a) == 12 and sum('mi_ode_rows_plugin.h' in s for s in a) == 6


def test_plan_reports_the_engine_or_the_refusal():
    y3 = torch.ones(5, 3, dtype=F64)
    for f, y0, lowered in ((rhs.Lorenz(), y3, None), (PC.van_der_pol(), torch.ones(5, 2, dtype=torch.float32), None),
                           (PC.time_callable, torch.ones(5, PC.TIME_DIM, dtype=F64), True)):
        for method, S in (('dopri5', 6), ('bosh3', 3), ('dopri8', 13), ('adaptive_heun', 1), ('tsit5', 6)):
            p = odeint.plan(f, y0, T5, method=method, options=ON)
            assert p['engine'] == 'fused' and p['kernel'].startswith('k_rows_rowlocal<%s, %d' % ('double' if y0.dtype == F64 else 'float', S)), p
            assert p['why'] == 'per-trajectory step control, one launch' and p['launches'] == 'one per call' and p['per_trajectory'] is True
            assert (p['lower'] is None) if lowered is None else (p['lower']['lowered'] is True and p['lower']['kind'] == 'rowlocal')
    for name, (f, y0, method, extra, fragment) in _refusals().items():
        if name.startswith('value_'):
            with pytest.raises(ValueError):
                odeint.plan(f, y0, T5, method=method, options=dict(ON, **extra))
            continue
        p = odeint.plan(f, y0, T5, method=method, options=dict(ON, **extra))
        assert p['engine'] == 'refused' and fragment in p['why'] and p['kernel'] is None, (name, p)
    assert 'k_persist_rowlocal' in odeint.plan(rhs.Lorenz(), y3, T5, method='dopri5')['kernel']          # the default is untouched
    assert 'k_persist_rowlocal' in odeint.plan(rhs.Lorenz(), y3, T5, method='dopri5', options={'per_trajectory': False})['kernel']


# ---- the per-row integration, compiled by g++ ------------------------------------------------------------------------------------------------
_LIBS = {}


def _host_lib(name):
    if name not in _LIBS:
        functor, dim = {'lorenz': (PC.LORENZ_FUNCTOR, 3), 'lv': (PC.LV_FUNCTOR, 2)}[name]
        d = tempfile.mkdtemp(prefix='per_trajectory_')
        os.makedirs(os.path.join(d, 'hip'))
        open(os.path.join(d, 'hip', 'hip_runtime.h'), 'w').close()
        cpp, so = os.path.join(d, name + '.cpp'), os.path.join(d, name + '.so')
        with open(cpp, 'w') as fh:
            fh.write(PC.host_source(functor, dim))
        res = subprocess.run(['g++', '-O1', '-ffp-contract=off', '-std=c++17', '-shared', '-fPIC', '-Wno-unknown-pragmas', '-I', d, '-I', N.CSRC,
                              cpp, '-o', so], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
        _LIBS[name] = C.CDLL(so)
    return _LIBS[name]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


METHODS = {'dopri5': (_DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID, 5, 4), 'bosh3': (_BOGACKI_SHAMPINE_TABLEAU, BS_C_MID, 3, 2)}


def _host_rows(name, method, y0, t, rtol, atol, scalars):
    tb, c_mid, order, init_order = METHODS[method]
    lib = _host_lib(name)
    f32 = lambda v: float(np.float64(np.float32(v)))       # noqa: E731  (dopri5.py:63-66: python float -> float32 -> float64)
    ctrl = np.array([rtol, atol, f32(0.9), f32(10.0), f32(0.2), np.nan, float(2 ** 31 - 1), order, init_order, N.CTRL_MISC, N.INTERP_QUARTIC_MID], dtype=np.float64)
    tab = PC.tableau_array(tb, c_mid)
    y0 = np.ascontiguousarray(y0, dtype=np.float64)
    batch, dim = y0.shape
    out = np.zeros((len(t) - 1, batch, dim))
    stats = np.zeros((batch, 4), dtype=np.int64)
    sc = np.zeros(8)
    sc[:len(scalars)] = scalars
    tt = np.ascontiguousarray(t, dtype=np.float64)
    rc = lib.rows_run(len(tb.alpha), 0, 1, _ptr(tab), _ptr(ctrl), _ptr(sc), C.c_longlong(batch), _ptr(y0), _ptr(tt), len(t), _ptr(out), _ptr(stats))
    assert rc == 0
    return np.concatenate([y0[None], out], axis=0), stats


def _band(got, ref, what):
    """tests/test_gpu_parity.py's band for the shared row-local kernel in float64 (RTOL, ATOL = 1e-5, 1e-6)."""
    bad = np.abs(got - ref) > 1e-6 + 1e-5 * np.abs(ref)
    assert not bad.any(), '%s: %d/%d outside band, max abs diff %.3e' % (what, bad.sum(), bad.size, np.abs(got - ref).max())


HOST_CASES = {
    ('lorenz', 'dopri5'): (lambda: PC.base_y0().numpy()[list(PC.BASE_ROWS)], PC.BASE_T, PC.lorenz_np, (10., 8. / 3., 28.)),
    ('lorenz', 'bosh3'): (lambda: PC.base_y0().numpy()[list(PC.BASE_ROWS)], PC.BASE_T * 0.05, PC.lorenz_np, (10., 8. / 3., 28.)),
    ('lv', 'dopri5'): (lambda: PC.lv_y0().numpy(), np.linspace(0., 2., 5), PC.lv_np, (1.5, 1.0, 3.0, 1.0)),
    ('lv', 'bosh3'): (lambda: PC.lv_y0().numpy(), np.linspace(0., 0.1, 5), PC.lv_np, (1.5, 1.0, 3.0, 1.0)),
}


@pytest.mark.parametrize('name,method', sorted(HOST_CASES))
def test_host_compiled_rows_equal_the_oracle_at_batch_one(name, method):
    """Every row of csrc/mi_ode_rows_core.h's integration (g++, float64) against oracle.ode_numpy.odeint(f, y0[i:i+1], t): attempt and accept
    counts exactly, the solution inside the band tests/test_gpu_parity.py gives the shared row-local kernel."""
    make, t, f_np, scalars = HOST_CASES[(name, method)]
    y0 = make()
    sol, stats = _host_rows(name if name != 'lv' else 'lv', method, y0, t, 1e-6, 1e-9, scalars)
    counts = []
    for i in range(y0.shape[0]):
        ref, st = O.odeint(f_np, y0[i:i + 1], t, rtol=1e-6, atol=1e-9, method=method, return_stats=True)
        assert (int(stats[i, 0]), int(stats[i, 1]), int(stats[i, 3])) == (st.n_attempts, st.n_accepted, 0), (i, stats[i], st.n_attempts, st.n_accepted)
        assert int(stats[i, 2]) == st.nfe, (i, stats[i], st.nfe)
        _band(sol[:, i:i + 1], ref, '%s %s row %d' % (name, method, i))
        counts.append(st.n_attempts)
    assert len(set(counts)) > 1, counts                      # the rows genuinely take different step sequences
    if (name, method) == ('lorenz', 'dopri5'):
        assert counts == [50, 47, 46, 43, 42, 39], counts
