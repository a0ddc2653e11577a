"""Gradients for per-trajectory solves (odeint_adjoint with options={'per_trajectory': True}, csrc/mi_ode_rows_adjoint.h) as far as the CPU
goes: the refusals and what the plans report, the C ABI, the generated vjp's rule for `t` against torch.autograd.grad, and one row's whole
backward - csrc/mi_ode_rows_adjoint_core.h compiled by g++ around the generated functor - held, row by row and interval by interval, to the
oracle's AdaptiveRK on the four-component tuple at batch 1 (attempt and accept counts exactly)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discrete_lowered_cases as DC                       # noqa: E402
import per_trajectory_adjoint_cases as AC                 # noqa: E402
import per_trajectory_cases as PC                         # noqa: E402
import test_lower_trace as TLT                            # noqa: E402
from tfdiffeq_amd import _native as N                     # noqa: E402
from tfdiffeq_amd import lower as L                       # noqa: E402
from tfdiffeq_amd import odeint, odeint_adjoint, rhs      # noqa: E402
from tfdiffeq_amd.bosh3 import _BOGACKI_SHAMPINE_TABLEAU, BS_C_MID   # noqa: E402
from tfdiffeq_amd.dopri5 import _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
T5 = torch.linspace(0., 1., 5, dtype=F64)
ON = AC.ON


# ---- refusals: a ValueError with the reason, decided without a device (every state here is a host tensor) -------------------------------
class _Tanh(torch.nn.Module):
    def __init__(self, dim, how='plain'):
        super(_Tanh, self).__init__()
        self.W = torch.nn.Parameter(torch.eye(dim, dtype=F64) * 0.3)
        self.b = torch.nn.Parameter(torch.zeros(dim, dtype=F64))
        self.how = how
        if how == 'unused':
            self.extra = torch.nn.Parameter(torch.ones(2, dtype=F64))

    def forward(self, t, y):
        W = self.W.t() if self.how == 'derived' else self.W
        return torch.tanh(y @ W + self.b) - 0.5 * y


class _PerRow(torch.nn.Module):
    def __init__(self, batch):
        super(_PerRow, self).__init__()
        self.c = torch.nn.Parameter(torch.full((batch, 3), 0.5, dtype=F64))

    def forward(self, t, y):
        return self.c * y * -1.0


class _Cumsum(torch.nn.Module):
    def forward(self, t, y):
        return torch.cumsum(y, -1)


class _TupleModule(torch.nn.Module):
    def forward(self, t, y):
        return (-y[0], -y[1])


def _refusals():
    g = torch.Generator().manual_seed(0)
    y3, y4, y5, y40 = (torch.randn(6, d, generator=g, dtype=F64) for d in (3, 4, 5, 40))
    lor = AC.LorenzModule()
    # name: (module, y0, method, options beyond the key, adjoint keywords, fragment)
    return {
        'rk4': (lor, y3, 'rk4', {}, {}, 'a fixed-grid or Adams method'),
        'lower_false': (lor, y3, 'dopri5', {'lower': False}, {}, "options['lower'] is False"),
        'sharded': (lor, y3, 'dopri5', {'process_group': object()}, {}, 'a sharded run'),
        'tracer_refuses': (_Cumsum(), y3, 'dopri5', {}, {}, 'the tracer refuses this callable'),
        'lowered_40_elements': (_Tanh(40), y40, 'dopri5', {}, {}, "a lowered 'coop' program, dim 40"),
        'forward_tableau': (lor, y3, 'dopri8', {}, {'adjoint_method': 'dopri8'}, "adjoint_method 'dopri8'"),
        'tuple_state': (_TupleModule(), (y3, y3), 'dopri5', {}, {}, 'a tuple state'),
        'n_aug': (_Tanh(5), y5, 'dopri5', {}, {}, 'N_aug = 2 * 5 + 1 + 30 = 41'),
        'adjoint_method': (lor, y3, 'dopri5', {}, {'adjoint_method': 'tsit5'}, "adjoint_method 'tsit5'"),
        'adjoint_method_default': (lor, y3, 'tsit5', {}, {}, "adjoint_method 'tsit5'"),
        'tuple_adjoint_rtol': (lor, y3, 'dopri5', {}, {'adjoint_rtol': (1e-6, 1e-6, 1e-6, 1e-6)}, 'tuple adjoint_rtol / adjoint_atol'),
        'tuple_adjoint_atol': (lor, y3, 'dopri5', {}, {'adjoint_atol': [1e-9] * 4}, 'tuple adjoint_rtol / adjoint_atol'),
        'adjoint_options': (lor, y3, 'dopri5', {}, {'adjoint_options': {'first_step': 0.1}}, "adjoint_options ['first_step']"),
        'forward_options_inherited': (lor, y3, 'dopri5', {'safety': 0.8}, {}, "adjoint_options ['safety']"),
        'derived_tensor': (_Tanh(4, 'derived'), y4, 'dopri5', {}, {}, 'a derived (non-leaf) trainable tensor'),
        'unused_parameter': (_Tanh(4, 'unused'), y4, 'dopri5', {}, {}, 'does not enter the trace as it is'),
        'batch_axes': (_PerRow(6), y3, 'dopri5', {}, {}, 'with batch axes'),
    }


@pytest.mark.parametrize('name', sorted(_refusals()))
def test_refusals_raise_value_error_with_the_reason(name):
    f, y0, method, extra, kw, fragment = _refusals()[name]
    with pytest.raises(ValueError) as e:
        odeint_adjoint(f, y0, T5, method=method, options=dict(ON, **extra), **kw)
    assert fragment in str(e.value), str(e.value)
    assert "options['per_trajectory'] refused" in str(e.value)
    p = odeint_adjoint.plan(f, y0, T5, method=method, options=dict(ON, **extra), **kw)
    assert p['engine'] == 'refused' and fragment in p['why'] and p['kernel'] is None, p


def test_what_is_not_a_refusal():
    lor, y3 = AC.LorenzModule(), torch.ones(4, 3, dtype=F64)
    with pytest.raises(ValueError) as e:                     # adjoint.py:187-188, before anything else
        odeint_adjoint(lambda t, y: -y, y3, T5, method='dopri5', options=ON)
    assert 'torch.nn.Module' in str(e.value)
    with pytest.raises(ValueError) as e:
        odeint_adjoint(lor, y3, T5, method='dopri5', options={'per_trajectory': 'yes'})
    assert 'must be True or False' in str(e.value)
    with pytest.raises(ValueError) as e:
        odeint_adjoint(lor, y3, T5, options=ON)
    assert 'without specifying `method`' in str(e.value)
    with pytest.raises(N.NativeError):                       # accepted (no ValueError): it is the device that is missing
        odeint_adjoint(lor, y3.clone().requires_grad_(True), T5, method='dopri5', options=ON)
    with pytest.raises(N.NativeError):
        odeint_adjoint(AC.TimeModule(), y3, T5, method='bosh3', options=ON, adjoint_options={'max_num_steps': 100})
    with pytest.raises(N.NativeError):                       # False: as if the key were absent - the existing route, the same host refusal
        odeint_adjoint(lor, y3, T5, method='dopri5', options={'per_trajectory': False})
    # plain odeint keeps refusing inputs that require grad, with the wording it had
    for f, y in ((lor, y3), (rhs.Lorenz(), y3.clone().requires_grad_(True))):
        with pytest.raises(ValueError) as e:
            odeint(f, y, T5, method='dopri5', options=ON)
        assert "options['per_trajectory'] refused" in str(e.value) and 'odeint_adjoint without the option' in str(e.value)


def test_plan_reports_the_kernel():
    y3 = torch.ones(5, 3, dtype=F64)
    for mod, y0, n_aug, P in ((AC.LorenzModule(), y3, 10, 3), (AC.TimeModule(torch.float32), y3.float(), 11, 4)):
        for method, S in (('dopri5', 6), ('bosh3', 3)):
            for p in (odeint.plan(mod, y0, T5, method=method, options=ON, adjoint=True), odeint_adjoint.plan(mod, y0, T5, method=method, options=ON),
                      odeint_adjoint.plan(mod, y0, T5, method='dopri5', adjoint_method=method, options=ON)):
                assert p['engine'] == 'fused' and p['kernel'].startswith('k_rows_adjoint<%s, %d' % ('double' if y0.dtype == F64 else 'float', S)), p
                assert p['launches'] == 'one per backward' and p['per_trajectory'] is True and p['n_aug'] == n_aug and p['n_params'] == P
                assert p['forward']['kernel'].startswith('k_rows_rowlocal<') and p['lower']['kind'] == 'rowlocal'
    with pytest.raises(ValueError):
        odeint_adjoint.plan(AC.LorenzModule(), y3, T5, method='dopri5')
    assert 'k_persist_rowlocal' in odeint.plan(rhs.Lorenz(), y3, T5, method='dopri5')['kernel']          # the default is untouched


# ---- header, exports, ABI ----------------------------------------------------------------------------------------------------------------
def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    assert 'int mi_ode_adjoint_rows(const mi_ode_adjoint_rows_desc* desc,' in header and 'mi_ode_adjoint_rows' in N.EXPORTED_SYMBOLS
    assert '#define MI_ODE_ABI_VERSION 13' in header and N.ABI_VERSION == 13
    lib = N.load()
    assert hasattr(lib, 'mi_ode_adjoint_rows') and lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_sizeof(0) == C.sizeof(N.Desc) == 2360 and lib.mi_ode_sizeof(1) == C.sizeof(N.Stats) == 88
    assert lib.mi_ode_adjoint_rows_sizeof() == C.sizeof(N.AdjointRowsDesc)
    plugin_h = open(os.path.join(N.CSRC, 'mi_ode_plugin.h')).read()
    rows_h = open(os.path.join(N.CSRC, 'mi_ode_rows.h')).read()
    assert '#define MI_ODE_PLUGIN_ABI 3' in plugin_h and '#define MI_ODE_ROWS_PLUGIN_ABI 1' in rows_h and 'adjoint' not in plugin_h
    assert lib.mi_ode_adjoint_rows(None, None, None, None, None, None, None, None, None) == N.E_INVALID
    d, r = N.AdjointRowsDesc(), N.Rhs()
    assert lib.mi_ode_adjoint_rows(C.byref(d), C.byref(r), None, None, None, None, None, None, None) == N.E_INVALID


def test_adjoint_source_is_a_translation_unit_of_its_own_kind():
    from tfdiffeq_amd import _plugin_build as PB
    tr = L.trace(AC.LorenzModule(), torch.zeros(2, 3, dtype=F64))
    src = L.adjoint_source(tr)
    assert '#include "mi_ode_rows_adjoint_plugin.h"' in src and 'MI_ODE_DEFINE_ROWS_ADJOINT_PLUGIN(mi::RhsUser)' in src
    assert 'static constexpr int D = 3;' in src and 'static constexpr int P = 3;' in src and 'tbar = ' in src
    roots = PB._source_roots(src)
    assert roots == ('mi_ode_rows_adjoint_plugin.h',)
    hashed = [os.path.basename(p) for p in PB._plugin_headers(roots)]
    assert 'mi_ode_rows_adjoint.h' in hashed and 'mi_ode_rows_adjoint_core.h' in hashed and 'mi_ode_rows_core.h' in hashed
    for default in ([os.path.basename(p) for p in PB._plugin_headers()], [os.path.basename(p) for p in PB._plugin_headers(('mi_ode_rows_plugin.h',))]):
        assert not any('adjoint' in h for h in default if h.startswith('mi_ode_rows')), default        # cached plugins are not rebuilt for this feature
    a, b = AC.adjoint_sources('cpu'), AC.adjoint_sources('cpu')
    assert a == b and len(a) == 12 and sum('mi_ode_rows_adjoint_plugin.h' in s for s in a) == 4 and sum('mi_ode_rows_plugin.h' in s for s in a) == 4


# ---- the rule for t ----------------------------------------------------------------------------------------------------------------------
def _compile(src, tag, extra=()):
    d = tempfile.mkdtemp(prefix='per_trajectory_adjoint_')
    os.makedirs(os.path.join(d, 'hip'))
    open(os.path.join(d, 'hip', 'hip_runtime.h'), 'w').close()
    cpp, so = os.path.join(d, tag + '.cpp'), os.path.join(d, tag + '.so')
    with open(cpp, 'w') as fh:
        fh.write(src)
    res = subprocess.run(['g++', '-O1', '-ffp-contract=off', '-std=c++17', '-shared', '-fPIC', '-Wno-unknown-pragmas', '-I', d, '-I', N.CSRC,
                          '-I', os.path.join(ROOT, 'include'), cpp, '-o', so] + list(extra), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return C.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _t_ops():
    s = torch.tensor(0.6, dtype=F64, requires_grad=True)
    v = torch.tensor([1., 2., 3.], dtype=F64, requires_grad=True)
    tm = AC.TimeModule()
    ops = {name: (f, ()) for name, (f, _frag) in TLT.OPS.items() if any(n.op == 't' for n in L.trace(f, torch.zeros(2, 3, dtype=F64)).live())}
    assert 'time' in ops
    ops.update({
        'time_trainable': (lambda t, y: y * torch.cos(t * s) + t ** 2 * v, (s, v)),
        'time_div_pow_exp': (lambda t, y: y / (1 + t * t) + torch.exp(-t * s) * torch.sin(y * t) + (t + 2) ** 0.5 * v + 2 ** t, (s, v)),
        'time_where_max': (lambda t, y: torch.where(y > 0, y * t, 0.1 * y) + torch.maximum(y, t * torch.ones_like(y)) + torch.tanh(t - y), ()),
        'time_sum': (lambda t, y: (y * t).sum(-1, keepdim=True) * torch.stack([y[..., 1], t * y[..., 0], y[..., 2] * s], dim=-1), (s,)),
        'time_module': (tm, tuple(tm.parameters())),
        'no_time': (lambda t, y: torch.sin(y) * s, (s,)),
    })
    return ops


@pytest.mark.parametrize('name', sorted(_t_ops()))
def test_the_rule_for_t_against_autograd(name):
    """ybar, tbar and the parameter contributions of the generated reverse code with the rule for the `t` node (g++, float64) against
    torch.autograd.grad of the callable itself, to the 1e-12 of DESIGN.md 11.1."""
    f, params = _t_ops()[name]
    y0 = torch.tensor(np.random.RandomState(0).randn(5, 3) * 0.7)
    tr = L.trace(f, y0)
    lib = _compile(L.host_vjp_t_source(tr), 'vjpt')
    pool, ps = AC.host_constants(tr)
    plist, P = L.vjp_params(tr)
    rng = np.random.RandomState(1)
    for r in range(y0.shape[0]):
        tt = 0.3 + 0.2 * r
        kbar = rng.randn(3)
        y = y0[r:r + 1].clone().requires_grad_(True)
        t_ = torch.tensor(tt, dtype=F64, requires_grad=True)
        out = f(t_, y)
        ref = torch.autograd.grad(out, (y, t_) + tuple(params), torch.tensor(kbar).reshape(out.shape), allow_unused=True)
        yin, ybar, tbar, tb = np.ascontiguousarray(y0[r].numpy()), np.zeros(3), np.full(1, np.nan), np.zeros(max(P, 1))
        lib.vjpt_f64(C.c_double(tt), _ptr(yin), _ptr(kbar), _ptr(ybar), _ptr(tbar), _ptr(tb), ps, _ptr(pool))
        gots = [ybar, tbar]
        refs = [np.zeros(3) if ref[0] is None else ref[0].reshape(-1).numpy(), np.zeros(1) if ref[1] is None else ref[1].reshape(-1).numpy()]
        for i, off, n in plist:
            k = [j for j, p in enumerate(params) if p is tr.tensors[i]['t']][0]
            refs.append(np.zeros(n) if ref[2 + k] is None else ref[2 + k].reshape(-1).numpy())
            gots.append(tb[off:off + n])
        for got, want in zip(gots, refs):
            assert np.all(np.abs(got - want) <= 1e-12 * (1 + np.abs(want))), (name, r, got, want)
        if name == 'no_time':
            assert tbar[0] == 0.0
        else:
            assert refs[1][0] != 0.0                         # (the case does exercise d/dt)


# sha256[:16] of lower.discrete_source / lower.host_vjp_source of tests/discrete_lowered_cases.SYSTEMS (float64, float32), recorded on the
# commit before the rule for t existed: plugins are cached by source hash, the rule must not change a byte of what was generated before
_SOURCE_HASHES = {
    'demo_net': ('087fb018d400b764', '226387d9159660fd', '1e3a60c7fcd74fed'),
    'lorenz': ('c00b6f1af59191fd', '2986f3ff147259a6', '6b2cb996975e321b'),
    'scalars': ('7f5d8bff58872d3b', '0a23a292cc04162e', 'afdefe93c1a49094'),
    'spiral': ('987448d01f9a02b1', '42021c660c7889ab', '47cb585e7fc5d85d'),
    'tanh8': ('c44ddd8fd8c8d8ec', '99f86d09e5156d89', 'eb6c2c79153f85de'),
}


def test_existing_generated_sources_are_unchanged():
    h = lambda s: hashlib.sha256(s.encode()).hexdigest()[:16]          # noqa: E731
    assert sorted(_SOURCE_HASHES) == sorted(DC.SYSTEMS)
    for name, (d64, d32, host) in _SOURCE_HASHES.items():
        for dt, want in ((torch.float64, d64), (torch.float32, d32)):
            f, _params, y0 = DC.SYSTEMS[name]('cpu', dt)
            tr = L.trace(f, y0)
            src = L.discrete_source(tr)
            assert h(src) == want and h(L.host_vjp_source(tr)) == host, (name, dt)
            assert 'tbar' not in src and 'tbar' in L.adjoint_source(tr)


# ---- one row's whole backward, compiled by g++ -------------------------------------------------------------------------------------------
_LIBS = {}
METHODS = {'dopri5': (_DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID, 5, 4), 'bosh3': (_BOGACKI_SHAMPINE_TABLEAU, BS_C_MID, 3, 2)}


def _host_backward(name, method, t, ans, g, rtol, atol, max_num_steps=2 ** 31 - 1):
    mod = AC.SYSTEMS[name][0]()
    tr = L.trace(mod, torch.zeros(2, 3, dtype=F64))
    if name not in _LIBS:
        _LIBS[name] = _compile(AC.host_source(tr), name)
    tb, c_mid, order, init_order = METHODS[method]
    f32 = lambda v: float(np.float64(np.float32(v)))       # noqa: E731  (dopri5.py:63-66: python float -> float32 -> float64)
    ctrl = np.array([rtol, atol, f32(0.9), f32(10.0), f32(0.2), float(max_num_steps), order, init_order], dtype=np.float64)
    tab = PC.tableau_array(tb, c_mid)
    pool, ps = AC.host_constants(tr)
    T, B, D = ans.shape
    P = L.vjp_params(tr)[1]
    out = dict(gy0=np.zeros((B, D)), rowp=np.zeros((B, P)), rowt=np.zeros((B, T)), counts=np.zeros((B, 3, T - 1), dtype=np.int64), status=np.zeros(B, dtype=np.int64))
    tt, ans, g = (np.ascontiguousarray(a, dtype=np.float64) for a in (t, ans, g))
    rc = _LIBS[name].adj_rows_run(len(tb.alpha), _ptr(tab), _ptr(ctrl), ps, _ptr(pool), C.c_longlong(B), T, _ptr(tt), _ptr(ans), _ptr(g), _ptr(out['gy0']),
                                  _ptr(out['rowp']), _ptr(out['rowt']), _ptr(out['counts']), _ptr(out['status']))
    assert rc == 0
    order_ = AC.compact_order(tr, list(mod.parameters()))
    out['rowp'] = np.concatenate([out['rowp'][:, off:off + n] for off, n in order_], axis=1)       # module order, as the twins return it
    return out, AC.SYSTEMS[name][1](mod)


def _band(got, ref, what):
    """tests/test_gpu_parity.py's band for the shared row-local kernel in float64 (RTOL, ATOL = 1e-5, 1e-6)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = np.abs(got - ref) > 1e-6 + 1e-5 * np.abs(ref)
    assert not bad.any(), '%s: %d/%d outside band, max abs diff %.3e' % (what, bad.sum(), bad.size, np.abs(got - ref).max())


# (system, method): rows, t, rtol, atol.  bosh3 takes a few hundred steps per interval at 1e-6 / 1e-9: its cases run at 1e-4 / 1e-7 on a
# short interval so that the oracle (Python, a row at a time) stays quick; the control logic exercised is the same
HOST_CASES = {
    ('lorenz', 'dopri5'): (PC.BASE_ROWS, PC.BASE_T, 1e-6, 1e-9),
    ('lorenz', 'bosh3'): (PC.BASE_ROWS, PC.BASE_T * 0.05, 1e-4, 1e-7),
    ('time', 'dopri5'): (tuple(range(9)), AC.TIME_T, 1e-6, 1e-9),
    ('time', 'bosh3'): (tuple(range(9)), AC.TIME_T, 1e-4, 1e-7),
}
# attempts of the intervals t_1 -> t_0 .. t_4 -> t_3 of the six BASE_ROWS (Lorenz, dopri5, 1e-6 / 1e-9), from the oracle
LORENZ_DOPRI5_ATTEMPTS = [[17, 15, 18, 17], [12, 12, 18, 20], [18, 23, 16, 13], [23, 19, 10, 12], [21, 16, 10, 15], [27, 18, 10, 12]]


@pytest.mark.parametrize('name,method', sorted(HOST_CASES))
def test_host_compiled_backward_equals_the_oracle_row_by_row(name, method):
    """Every row and every interval of csrc/mi_ode_rows_adjoint_core.h's backward (g++, float64) against oracle.ode_numpy's AdaptiveRK on
    the tuple (y [1, D], adj_y [1, D], adj_t [], adj_params [P]) of that row alone: attempts, accepted steps and function evaluations
    exactly, gradients inside the float64 band of the per-trajectory tests.  A loss that reads every output time: the jumps take part."""
    rows, t, rtol, atol = HOST_CASES[(name, method)]
    y0 = AC.SYSTEMS[name][4]().numpy()[list(rows)]
    theta = AC.SYSTEMS[name][1](AC.SYSTEMS[name][0]())
    ans = AC.oracle_forward(name, theta, y0, t, rtol, atol, method)
    g = AC.cotangent(ans)
    got, theta = _host_backward(name, method, t, ans, g, rtol, atol)
    assert not got['status'].any()
    attempts = []
    for i in range(y0.shape[0]):
        gy, gp, tv, att, acc, nfe = AC.oracle_backward(name, theta, t, ans[:, i], g[:, i], rtol, atol, method)
        assert got['counts'][i, 0].tolist() == att and got['counts'][i, 1].tolist() == acc and got['counts'][i, 2].tolist() == nfe, (i, got['counts'][i], att, acc, nfe)
        _band(got['gy0'][i], gy, '%s %s row %d grad_y0' % (name, method, i))
        _band(got['rowp'][i], gp, '%s %s row %d grad_params' % (name, method, i))
        _band(got['rowt'][i], tv, '%s %s row %d time_vjps' % (name, method, i))
        attempts.append(att)
    assert len(set(tuple(a) for a in attempts)) > 1, attempts          # the rows genuinely take different step sequences
    if (name, method) == ('lorenz', 'dopri5'):
        assert attempts == LORENZ_DOPRI5_ATTEMPTS, attempts


def test_host_compiled_backward_last_output_only_and_a_row_that_cannot_finish():
    name, method = 'lorenz', 'dopri5'
    rows, t, rtol, atol = HOST_CASES[(name, method)]
    y0 = AC.SYSTEMS[name][4]().numpy()[list(rows)]
    theta = AC.SYSTEMS[name][1](AC.SYSTEMS[name][0]())
    ans = AC.oracle_forward(name, theta, y0, t, rtol, atol, method)
    g = AC.cotangent(ans, every=False)                       # a loss that reads the last output only: every dLd_cur_t but the last is zero
    got, theta = _host_backward(name, method, t, ans, g, rtol, atol)
    for i in (0, 3):
        gy, gp, tv, att, acc, nfe = AC.oracle_backward(name, theta, t, ans[:, i], g[:, i], rtol, atol, method)
        assert got['counts'][i, 0].tolist() == att and got['counts'][i, 1].tolist() == acc
        _band(got['gy0'][i], gy, 'grad_y0')
        _band(got['rowp'][i], gp, 'grad_params')
        _band(got['rowt'][i], tv, 'time_vjps')
        assert np.all(got['rowt'][i, 1:-1] == 0.0) and got['rowt'][i, -1] != 0.0
    # max_num_steps = 3: the first interval of every row ends by attempt_tail's status exit after 3 attempts, the row stops there
    got, _ = _host_backward(name, method, t, ans, AC.cotangent(ans), rtol, atol, max_num_steps=3)
    assert np.all(got['status'] == N.ST_MAX_STEPS)
    assert np.all(got['counts'][:, 0, -1] == 3) and np.all(got['counts'][:, 0, :-1] == 0)
    with pytest.raises(AssertionError) as e:
        AC.oracle_backward(name, theta, t, ans[:, 0], AC.cotangent(ans)[:, 0], rtol, atol, method, max_num_steps=3)
    assert 'max_num_steps exceeded (3>=3)' in str(e.value)
