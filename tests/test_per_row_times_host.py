"""Per-row output times, lengths and tolerances under options={'per_trajectory': True} (a 2-D `t`, options['t_lengths'], [batch] rtol /
atol; csrc/mi_ode_rows_t.h) as far as the CPU goes: the per-row integration fed per-row times - csrc/mi_ode_rows_core.h
compiled by g++ and held, row by row, to the oracle's batch-1 solve -, the refusals and validation errors, the route of a 1-D `t`, what
`odeint.plan` reports, the C ABI, and the generated sources of the kinds that existed before.

The host cases.  Every row has its own horizon, its own length (cycling through 1 .. T, so lengths 1 and 2 occur) and its own tolerances
(the method's base rtol / atol times 1, 10^-0.5 or 10^-1 by row).  Horizons and base tolerances are chosen per method so that the oracle
needs at most a few hundred attempts per row (the low-order methods get short horizons and loose tolerances, as tests/test_gpu_per_trajectory.py
`LV_CASES` does).  Attempts, accepted steps and function evaluations are held exactly; values inside `band64` of tests/test_gpu_per_trajectory.py."""
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
import per_row_times_cases as RC                           # noqa: E402
import per_trajectory_cases as PC                          # noqa: E402
from oracle import ode_numpy as O                         # noqa: E402
from tfdiffeq_amd import _native as N                     # noqa: E402
from tfdiffeq_amd import dispatch as D                    # noqa: E402
from tfdiffeq_amd import odeint, odeint_adjoint, rhs      # noqa: E402
from tfdiffeq_amd.odeint import SOLVERS                   # noqa: E402
from tfdiffeq_amd.solvers import _is_fsal_shaped          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
ON = {'per_trajectory': True}


def band64(got, ref, what):
    """`band64` of tests/test_gpu_per_trajectory.py (that module is marked gpu as a whole; the band is restated, not widened)."""
    bad = np.abs(got - ref) > 1e-6 + 1e-5 * np.abs(ref)
    assert not bad.any(), '%s: %d/%d outside band, max abs diff %.3e' % (what, bad.sum(), bad.size, np.abs(got - ref).max())


# ---- the per-row integration with per-row times, compiled by g++ ---------------------------------------------------------------------------
_LIBS = {}


def _host_lib(name):
    if name not in _LIBS:
        functor, dim = {'lorenz': (PC.LORENZ_FUNCTOR, 3), 'lv': (PC.LV_FUNCTOR, 2)}[name]
        d = tempfile.mkdtemp(prefix='per_row_times_')
        os.makedirs(os.path.join(d, 'hip'))
        open(os.path.join(d, 'hip', 'hip_runtime.h'), 'w').close()
        cpp, so = os.path.join(d, name + '.cpp'), os.path.join(d, name + '.so')
        with open(cpp, 'w') as fh:
            fh.write(RC.host_source_t(functor, dim))
        res = subprocess.run(['g++', '-O1', '-ffp-contract=off', '-std=c++17', '-shared', '-fPIC', '-Wno-unknown-pragmas', '-I', d, '-I', N.CSRC,
                              cpp, '-o', so], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
        _LIBS[name] = C.CDLL(so)
    return _LIBS[name]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_rows_t(name, method, y0, t, lengths, rtol, atol, scalars):
    from tfdiffeq_amd.misc import _TupleFunc
    cls = SOLVERS[method](_TupleFunc(rhs.Lorenz()), (torch.ones(1, 3, dtype=F64),), rtol=1e-6, atol=1e-9)      # (the solver's tableau, orders, controller)
    tb = cls.tableau
    lib = _host_lib(name)
    f32 = lambda v: float(np.float64(np.float32(v)))       # noqa: E731  (dopri5.py:63-66: python float -> float32 -> float64)
    ctrl = np.array([0., 0., f32(0.9), f32(10.0), f32(0.2), np.nan, float(2 ** 31 - 1), cls.order, cls.init_order, cls.controller, cls.interp],
                    dtype=np.float64)
    tab = PC.tableau_array(tb, cls.c_mid)
    y0 = np.ascontiguousarray(y0, dtype=np.float64)
    batch, dim = y0.shape
    T = t.shape[1]
    out = np.zeros((T - 1, batch, dim))
    stats = np.zeros((batch, 4), dtype=np.int64)
    sc = np.zeros(8)
    sc[:len(scalars)] = scalars
    tt, ll = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(lengths, dtype=np.int32)
    rr, aa = np.ascontiguousarray(rtol, dtype=np.float64), np.ascontiguousarray(atol, dtype=np.float64)
    rc = lib.rows_run_t(len(tb.alpha), int(cls.interp != N.INTERP_QUARTIC_MID), int(_is_fsal_shaped(tb)), _ptr(tab), _ptr(ctrl), _ptr(sc),
                        C.c_longlong(batch), _ptr(y0), _ptr(tt), T, _ptr(ll), _ptr(rr), _ptr(aa), _ptr(out), _ptr(stats))
    assert rc == 0
    return np.concatenate([y0[None], out], axis=0), stats


# method -> (horizon scale, base rtol, base atol, oracle options)
HOST_METHODS = {
    'dopri5': (1.0, 1e-6, 1e-9, None),
    'tsit5': (1.0, 1e-6, 1e-9, {'tsit5_fixed': True}),
    'bosh3': (0.1, 1e-4, 1e-7, None),
    'dopri8': (1.0, 1e-6, 1e-9, None),
    'adaptive_heun': (0.05, 1e-3, 1e-6, None),
}
HOST_SYSTEMS = {
    'lorenz': (lambda: PC.base_y0().numpy(), PC.lorenz_np, (10., 8. / 3., 28.), 1.0),
    'lv': (lambda: PC.lv_y0().numpy(), PC.lv_np, (1.5, 1.0, 3.0, 1.0), 2.0),
}


@pytest.mark.parametrize('method', sorted(HOST_METHODS))
@pytest.mark.parametrize('name', sorted(HOST_SYSTEMS))
def test_host_compiled_rows_with_their_own_times_equal_the_oracle_at_batch_one(name, method):
    make, f_np, scalars, end = HOST_SYSTEMS[name]
    scale, rtol0, atol0, oopts = HOST_METHODS[method]
    y0 = make()
    batch = y0.shape[0]
    t, lengths = RC.ragged(batch, T=6, end=end * scale)
    assert 1 in lengths and 2 in lengths
    tighten = 10.0 ** (-0.5 * (np.arange(batch) % 3))
    rtol, atol = rtol0 * tighten, atol0 * tighten
    sol, stats = _host_rows_t(name, method, y0, t, lengths, rtol, atol, scalars)
    counts = []
    for i in range(batch):
        n = int(lengths[i])
        assert int(stats[i, 3]) == 0, (i, stats[i])
        assert not sol[n:, i].any()                          # (nothing is written past the row's own length)
        if n == 1:                                           # only y0: the two evaluations of the initial step, no attempt
            assert (int(stats[i, 0]), int(stats[i, 1])) == (0, 0), (i, stats[i])
            continue
        ref, st = O.odeint(f_np, y0[i:i + 1], t[i, :n], rtol=float(rtol[i]), atol=float(atol[i]), method=method, options=oopts, return_stats=True)
        assert (int(stats[i, 0]), int(stats[i, 1])) == (st.n_attempts, st.n_accepted), (i, n, stats[i], st.n_attempts, st.n_accepted)
        if method != 'tsit5':                                # (the oracle's tsit5 counts its dense-output evaluations its own way)
            assert int(stats[i, 2]) == st.nfe, (i, stats[i], st.nfe)
        band64(sol[:n, i:i + 1], ref, '%s %s row %d' % (name, method, i))
        counts.append(st.n_attempts)
    assert len(set(counts)) > 1, counts


# ---- refusals and validation: decided without a device (every state here is a host tensor) ---------------------------------------------------------
def _t2(batch=6, T=5):
    return torch.as_tensor(RC.horizon_t(batch, T))


def _bad_inputs():
    g = torch.Generator().manual_seed(0)
    y3 = torch.randn(6, 3, generator=g, dtype=F64)
    lor = rhs.Lorenz()
    mixed, crooked = _t2(), _t2()
    mixed[2] = -mixed[2]
    crooked[4, 3] = crooked[4, 2]
    nan_pad = _t2()
    nan_pad[:, 3:] = float('nan')
    return {
        # name: (func, y0, t, tolerances, options, exception, fragment)
        't_first_axis': (lor, y3, _t2(5), {}, {}, ValueError, '`t` of shape (5, 5) for a state of 6 rows'),
        't_three_axes': (lor, y3, torch.zeros(6, 5, 1, dtype=F64), {}, {}, ValueError, '`t` of shape (6, 5, 1)'),
        'state_not_2d': (lor, torch.zeros(2, 3, 3, dtype=F64), _t2(2), {}, {}, ValueError, 'belongs to row i of a [batch, dim] state'),
        'lengths_without_2d_t': (lor, y3, torch.linspace(0., 1., 5, dtype=F64), {}, {'t_lengths': torch.full((6,), 3)}, ValueError,
                                 "options['t_lengths'] needs a 2-D `t`"),
        'lengths_shape': (lor, y3, _t2(), {}, {'t_lengths': torch.full((5,), 3)}, ValueError, "options['t_lengths'] of shape (5,)"),
        'lengths_float': (lor, y3, _t2(), {}, {'t_lengths': torch.full((6,), 3.)}, ValueError, 'must be an integer tensor of shape [batch]'),
        'lengths_zero': (lor, y3, _t2(), {}, {'t_lengths': torch.tensor([5, 5, 0, 5, 5, 5])}, ValueError, 'must lie in 1 .. T = 5: row 2 has 0'),
        'lengths_past_T': (lor, y3, _t2(), {}, {'t_lengths': torch.tensor([5, 5, 5, 5, 5, 6])}, ValueError, 'must lie in 1 .. T = 5: row 5 has 6'),
        'rtol_shape': (lor, y3, _t2(), {'rtol': torch.full((5,), 1e-6)}, {}, ValueError, '`rtol` of shape (5,) for a state of 6 rows'),
        'atol_shape_1d_t': (lor, y3, torch.linspace(0., 1., 5, dtype=F64), {'atol': torch.full((6, 1), 1e-9)}, {}, ValueError,
                            '`atol` of shape (6, 1) for a state of 6 rows'),
        'mixed_directions': (lor, y3, mixed, {}, {}, ValueError, 'run in different directions (row 0 increases, row 2 decreases)'),
        'not_monotone': (lor, y3, crooked, {}, {}, AssertionError, 't must be strictly increasing or decrasing [per_trajectory: row 4'),
        'nan_inside_the_length': (lor, y3, nan_pad, {}, {'t_lengths': torch.full((6,), 4)}, AssertionError, '[per_trajectory: row 0'),
        'integer_t': (lor, y3, torch.arange(30).reshape(6, 5), {}, {}, TypeError, '`t` must be a floating point Tensor'),
        'lowered_t_first_axis': (PC.time_callable, torch.ones(6, PC.TIME_DIM, dtype=F64), _t2(5), {}, {}, ValueError, '`t` of shape (5, 5)'),
        'euler': (lor, y3, _t2(), {}, {}, ValueError, 'a fixed-grid or Adams method'),
        'linear': (rhs.Linear(torch.eye(8, dtype=F64)), torch.ones(6, 8, dtype=F64), _t2(), {}, {}, ValueError, 'matrix-core or cooperative kernels (Linear, dim 8)'),
    }


@pytest.mark.parametrize('name', sorted(_bad_inputs()))
def test_refusals_and_validation_errors_carry_the_reason(name):
    f, y0, t, tol, extra, exc, fragment = _bad_inputs()[name]
    with pytest.raises(exc) as e:
        odeint(f, y0, t, method='euler' if name == 'euler' else 'dopri5', options=dict(ON, **extra), **tol)
    assert fragment in str(e.value), str(e.value)
    if exc is ValueError and name != 'lengths_without_2d_t':
        assert "options['per_trajectory'] refused" in str(e.value)


def test_valid_per_row_inputs_pass_validation_and_only_the_device_is_missing():
    """NaN beyond a row's length is never looked at; all rows decreasing is a direction; lengths of 1 have no direction at all."""
    y3 = torch.ones(6, 3, dtype=F64)
    t, lengths = RC.ragged(6, T=4)
    for tt, opts, tol in ((torch.as_tensor(t), {'t_lengths': torch.as_tensor(lengths)}, {}),
                          (-torch.as_tensor(t), {'t_lengths': torch.as_tensor(lengths).long()}, {}),
                          (_t2(), {}, {'rtol': torch.full((6,), 1e-5), 'atol': 1e-8}),
                          (RC.horizon_t(6, 5).tolist(), {}, {}),                     # (times as nested lists)
                          (torch.linspace(0., 1., 5), {}, {'rtol': 1e-5, 'atol': torch.full((6,), 1e-8, dtype=torch.float32)}),
                          (_t2(), {'t_lengths': torch.ones(6, dtype=torch.int32)}, {})):
        with pytest.raises(N.NativeError):                   # accepted (no ValueError): it is the device that is missing
            odeint(rhs.Lorenz(), y3, tt, method='dopri5', options=dict(ON, **opts), **tol)
    from tfdiffeq_amd import rows_times
    rt, opts = rows_times.prepare(y3, -torch.as_tensor(t), 1e-6, torch.full((6,), 1e-8), dict(ON, t_lengths=torch.as_tensor(lengths)))
    assert rt.decreasing and rt.T == 4 and 't_lengths' not in opts and rt.rtol is None and rt.rtol0 == 1e-6 and rt.atol.dtype == F64
    assert rt.t.dtype == F64 and rt.lengths.dtype == torch.int32 and torch.equal(rt.t[3, :4], torch.as_tensor(t)[3, :4])   # (the sign is taken out)
    assert rows_times.prepare(y3, torch.linspace(0., 1., 5), 1e-6, 1e-9, ON) == (None, ON)


def test_a_1d_t_with_scalar_tolerances_still_reaches_the_old_route():
    from tfdiffeq_amd.misc import _TupleFunc
    y = torch.ones(4, 3, dtype=F64)
    c = SOLVERS['dopri5'](_TupleFunc(rhs.Lorenz()), (y,), rtol=1e-6, atol=1e-9, per_trajectory=True)
    assert c.route().kind == 'fused_rows' and c.route().why == D.ROWS_WHY == 'per-trajectory step control, one launch'
    assert D.rows_t_wanted((5,), None, None, False) is False and D.rows_t_wanted((5,), (), (), False) is False
    assert D.rows_t_wanted((4, 5), None, None, False) and D.rows_t_wanted((5,), (4,), None, False) and D.rows_t_wanted((5,), None, (4,), False)
    assert D.rows_t_wanted((4, 5), None, None, True)
    with pytest.raises(ValueError):
        D.rows_t_wanted((5,), None, None, True)
    assert D.rows_t_refusal((4, 3), (4, 5), (4,), True, (4,), None) == ''
    p = odeint.plan(rhs.Lorenz(), y, torch.linspace(0., 1., 5), method='dopri5', options=ON)
    assert p['kernel'].startswith('k_rows_rowlocal<double, 6') and p['why'] == D.ROWS_WHY


# ---- plans ----------------------------------------------------------------------------------------------------------------------------------
def test_plan_reports_the_t_kernel_or_the_refusal():
    y3 = torch.ones(6, 3, dtype=F64)
    for f, y0, lowered in ((rhs.Lorenz(), y3, None), (PC.van_der_pol(), torch.ones(6, 2, dtype=torch.float32), None),
                           (PC.time_callable, torch.ones(6, PC.TIME_DIM, dtype=F64), True)):
        for method, S in (('dopri5', 6), ('bosh3', 3), ('dopri8', 13), ('adaptive_heun', 1), ('tsit5', 6)):
            for t, tol, extra in ((_t2(), {}, {}), (_t2(), {}, {'t_lengths': torch.full((6,), 2)}), (torch.linspace(0., 1., 5), {'rtol': torch.full((6,), 1e-5)}, {})):
                p = odeint.plan(f, y0, t, method=method, options=dict(ON, **extra), **tol)
                assert p['engine'] == 'fused' and p['kernel'].startswith('k_rows_rowlocal_t<%s, %d' % ('double' if y0.dtype == F64 else 'float', S)), p
                assert p['why'] == D.ROWS_T_WHY and p['launches'] == 'one per call' and p['per_trajectory'] is True
                assert (p['lower'] is None) if lowered is None else (p['lower']['lowered'] is True and p['lower']['kind'] == 'rowlocal')
    for name, (f, y0, t, tol, extra, exc, fragment) in _bad_inputs().items():
        if exc is not ValueError or name in ('lengths_zero', 'lengths_past_T', 'mixed_directions'):        # (values: the call checks them, not the plan)
            continue
        p = odeint.plan(f, y0, t, method='euler' if name == 'euler' else 'dopri5', options=dict(ON, **extra), **tol)
        assert p['engine'] == 'refused' and fragment in p['why'] and p['kernel'] is None, (name, p)


def test_the_gradient_route_plans_the_t_kernels_and_refuses_with_the_reason():
    """odeint_adjoint takes the same per-row inputs: `odeint_adjoint.plan` reports k_rows_adjoint_t behind k_rows_rowlocal_t; shapes, values
    and decreasing rows are refused before a device is asked for; a 1-D t with scalar tolerances plans the old kernels."""
    import per_trajectory_adjoint_cases as AC
    m = AC.LorenzModule()
    y0 = torch.ones(6, 3, dtype=F64)
    t1 = torch.linspace(0., 1., 5)
    for t, tol, extra in ((_t2(), {}, {}), (_t2(), {}, {'t_lengths': torch.full((6,), 2)}), (t1, {'rtol': torch.full((6,), 1e-5)}, {}),
                          (t1, {'adjoint_atol': torch.full((6,), 1e-8)}, {})):
        for method, S in (('dopri5', 6), ('bosh3', 3)):
            p = odeint_adjoint.plan(m, y0, t, method=method, options=dict(ON, **extra), **tol)
            assert p['engine'] == 'fused' and p['kernel'].startswith('k_rows_adjoint_t<double, %d' % S) and p['why'] == D.ROWS_ADJOINT_T_WHY, p
            assert p['launches'] == 'one per backward' and p['n_aug'] == 10 and p['n_params'] == 3
            if 'adjoint_atol' not in tol:
                assert p['forward']['kernel'].startswith('k_rows_rowlocal_t<double, %d' % S), p['forward']
        with pytest.raises(N.NativeError):                   # accepted (no ValueError): it is the device that is missing
            odeint_adjoint(m, y0, t, method='dopri5', options=dict(ON, **extra), **tol)
    p = odeint_adjoint.plan(m, y0, t1, method='dopri5', options=ON)
    assert p['kernel'].startswith('k_rows_adjoint<double, 6') and p['why'] == D.ROWS_ADJOINT_WHY and p['forward']['kernel'].startswith('k_rows_rowlocal<')
    crooked = _t2()
    crooked[4, 3] = crooked[4, 2]
    for t, tol, extra, exc, fragment in (
            (_t2(5), {}, {}, ValueError, '`t` of shape (5, 5) for a state of 6 rows'),
            (_t2(), {'adjoint_rtol': torch.full((5,), 1e-6)}, {}, ValueError, '`adjoint_rtol` of shape (5,) for a state of 6 rows'),
            (t1, {}, {'t_lengths': torch.full((6,), 3)}, ValueError, "options['t_lengths'] needs a 2-D `t`"),
            (_t2(), {}, {'t_lengths': torch.tensor([5, 5, 0, 5, 5, 5])}, ValueError, 'must lie in 1 .. T = 5: row 2 has 0'),
            (-_t2(), {}, {}, ValueError, 'decreasing rows of `t`'),
            (crooked, {}, {}, AssertionError, '[per_trajectory: row 4')):
        with pytest.raises(exc) as e:
            odeint_adjoint(m, y0, t, method='dopri5', options=dict(ON, **extra), **tol)
        assert fragment in str(e.value), str(e.value)
        if exc is ValueError and 'needs a 2-D' not in fragment:
            assert "options['per_trajectory'] refused" in str(e.value)
    p = odeint_adjoint.plan(m, y0, _t2(5), method='dopri5', options=ON)
    assert p['engine'] == 'refused' and '`t` of shape (5, 5)' in p['why']


# ---- one row's whole backward with its own times, compiled by g++ ------------------------------------------------------------------------------
def _host_backward_t(name, method, t, lengths, rtol, atol, ans, g):
    import per_trajectory_adjoint_cases as AC
    from tfdiffeq_amd import lower as L
    from tfdiffeq_amd.rows_adjoint import _tableau
    mod = AC.SYSTEMS[name][0]()
    tr = L.trace(mod, torch.zeros(2, 3, dtype=F64))
    key = 'adjoint_' + name
    if key not in _LIBS:
        d = tempfile.mkdtemp(prefix='per_row_times_adjoint_')
        os.makedirs(os.path.join(d, 'hip'))
        open(os.path.join(d, 'hip', 'hip_runtime.h'), 'w').close()
        cpp, so = os.path.join(d, name + '.cpp'), os.path.join(d, name + '.so')
        with open(cpp, 'w') as fh:
            fh.write(RC.host_adjoint_source_t(tr))
        res = subprocess.run(['g++', '-O1', '-ffp-contract=off', '-std=c++17', '-shared', '-fPIC', '-Wno-unknown-pragmas', '-I', d, '-I', N.CSRC,
                              '-I', os.path.join(ROOT, 'include'), cpp, '-o', so], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
        _LIBS[key] = C.CDLL(so)
    tb, c_mid, order, init_order = _tableau(method)
    f32 = lambda v: float(np.float64(np.float32(v)))       # noqa: E731  (dopri5.py:63-66: python float -> float32 -> float64)
    ctrl = np.array([0., 0., f32(0.9), f32(10.0), f32(0.2), float(2 ** 31 - 1), order, init_order], dtype=np.float64)
    tab = PC.tableau_array(tb, c_mid)
    pool, ps = AC.host_constants(tr)
    T, B, Dm = ans.shape
    P = L.vjp_params(tr)[1]
    out = dict(gy0=np.zeros((B, Dm)), rowp=np.zeros((B, P)), rowt=np.full((B, T), np.nan), counts=np.zeros((B, 3 * (T - 1)), dtype=np.int64),
               status=np.zeros(B, dtype=np.int64))
    tt, ans, g, rr, aa = (np.ascontiguousarray(a, dtype=np.float64) for a in (t, ans, g, rtol, atol))
    ll = np.ascontiguousarray(lengths, dtype=np.int32)
    rc = _LIBS[key].adj_rows_run_t(len(tb.alpha), _ptr(tab), _ptr(ctrl), ps, _ptr(pool), C.c_longlong(B), T, _ptr(tt), _ptr(ll), _ptr(rr), _ptr(aa),
                                   _ptr(ans), _ptr(g), _ptr(out['gy0']), _ptr(out['rowp']), _ptr(out['rowt']), _ptr(out['counts']), _ptr(out['status']))
    assert rc == 0
    order_ = AC.compact_order(tr, list(mod.parameters()))
    out['rowp'] = np.concatenate([out['rowp'][:, off:off + n] for off, n in order_], axis=1)       # module order, as the twins return it
    return out, AC.SYSTEMS[name][1](mod)


# (system, method): rows, rtol, atol, the factor on the system's own interval - bosh3 as in tests/test_per_trajectory_adjoint_host.py
HOST_ADJOINT_CASES = {
    ('lorenz', 'dopri5'): (PC.BASE_ROWS, 1e-6, 1e-9, 1.0),
    ('lorenz', 'bosh3'): (PC.BASE_ROWS, 1e-4, 1e-7, 0.05),
    ('time', 'dopri5'): (tuple(range(9)), 1e-6, 1e-9, 1.0),
    ('time', 'bosh3'): (tuple(range(9)), 1e-4, 1e-7, 1.0),
}


@pytest.mark.parametrize('name,method', sorted(HOST_ADJOINT_CASES))
def test_host_compiled_backward_with_per_row_times_equals_the_oracle_row_by_row(name, method):
    """rows_adjoint_row (csrc/mi_ode_rows_adjoint_core.h, g++, float64), called as a lane of k_rows_adjoint_t calls it - its own negated
    times, its own length, its own tolerances - against oracle.ode_numpy on the four-component tuple of that row alone over t[i, :len_i]:
    attempts, accepted steps and function evaluations of every interval exactly, gradients inside the float64 band.  Lengths 1 .. T with
    NaN in the padding of t; the padding of the solution and of the cotangent holds NaN too: none of it is read."""
    import per_trajectory_adjoint_cases as AC
    rows, rtol0, atol0, factor = HOST_ADJOINT_CASES[(name, method)]
    y0 = AC.SYSTEMS[name][4]().numpy()[list(rows)]
    B, T = y0.shape[0], 5
    t, lengths = RC.ragged_adjoint_t(name, B, T)
    t = t[:, :1] + (t - t[:, :1]) * factor
    tighten = 10.0 ** (-0.5 * (np.arange(B) % 3))
    rtol, atol = rtol0 * tighten, atol0 * tighten
    theta = AC.SYSTEMS[name][1](AC.SYSTEMS[name][0]())
    ans = np.full((T, B, 3), np.nan)
    for i in range(B):
        n = int(lengths[i])
        ans[:n, i:i + 1] = AC.oracle_forward(name, theta, y0[i:i + 1], t[i, :n], float(rtol[i]), float(atol[i]), method) if n > 1 else y0[None, i:i + 1]
    g = AC.cotangent(ans)                                     # (NaN where ans is)
    got, theta = _host_backward_t(name, method, t, lengths, rtol, atol, ans, g)
    assert not got['status'].any()
    attempts = []
    for i in range(B):
        n = int(lengths[i])
        gy, gp, tv, att, acc, nfe = AC.oracle_backward(name, theta, t[i, :n], ans[:n, i], g[:n, i], float(rtol[i]), float(atol[i]), method)
        counts = got['counts'][i, :3 * (n - 1)].reshape(3, n - 1)          # (packed by the row's own length, as rows_adjoint_row leaves them)
        assert counts[0].tolist() == att and counts[1].tolist() == acc and counts[2].tolist() == nfe, (i, n, counts, att, acc, nfe)
        assert not got['counts'][i, 3 * (n - 1):].any() and np.isnan(got['rowt'][i, n:]).all()      # nothing is written past the row's length
        band64(got['gy0'][i], gy, '%s %s row %d grad_y0' % (name, method, i))
        band64(got['rowp'][i], gp, '%s %s row %d grad_params' % (name, method, i))
        band64(got['rowt'][i, :n], tv, '%s %s row %d time_vjps' % (name, method, i))
        attempts.append(tuple(att))
    assert len(set(attempts)) > 1, attempts


# ---- header, exports, ABI, generated sources ---------------------------------------------------------------------------------------------------
def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    assert 'int mi_ode_integrate_rows_t(mi_ode_handle h,' in header and 'mi_ode_integrate_rows_t' in N.EXPORTED_SYMBOLS
    assert '#define MI_ODE_ABI_VERSION 13' in header and N.ABI_VERSION == 13
    lib = N.load()
    assert hasattr(lib, 'mi_ode_integrate_rows_t') and lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_sizeof(0) == C.sizeof(N.Desc) == 2360 and lib.mi_ode_sizeof(1) == C.sizeof(N.Stats) == 88
    assert '#define MI_ODE_PLUGIN_ABI 3' in open(os.path.join(N.CSRC, 'mi_ode_plugin.h')).read()
    assert '#define MI_ODE_ROWS_PLUGIN_ABI 1' in open(os.path.join(N.CSRC, 'mi_ode_rows.h')).read()
    assert '#define MI_ODE_ROWS_T_PLUGIN_ABI 1' in open(os.path.join(N.CSRC, 'mi_ode_rows_t.h')).read()
    assert lib.mi_ode_integrate_rows_t(None, None, None, None, 0, None, None, None, None, None, None, None) == N.E_INVALID
    makefile = open(os.path.join(N.CSRC, 'Makefile')).read()
    assert ' mi_ode_rows_t ' in makefile and ' mi_ode_rows_t_f32' in makefile and ' mi_ode_rows_adjoint_t' in makefile
    # the gradient entry point: its own descriptor with a layout check, the existing one untouched
    assert 'int mi_ode_adjoint_rows_t(const mi_ode_adjoint_rows_t_desc* desc,' in header and 'mi_ode_adjoint_rows_t' in N.EXPORTED_SYMBOLS
    assert lib.mi_ode_adjoint_rows_t_sizeof() == C.sizeof(N.AdjointRowsTDesc) == C.sizeof(N.AdjointRowsDesc) + 3 * C.sizeof(C.c_void_p)
    assert lib.mi_ode_adjoint_rows_sizeof() == C.sizeof(N.AdjointRowsDesc)
    assert '#define MI_ODE_ROWS_ADJOINT_PLUGIN_ABI 0x41520001' in open(os.path.join(N.CSRC, 'mi_ode_rows_adjoint.h')).read()
    assert '#define MI_ODE_ROWS_ADJOINT_T_PLUGIN_ABI 0x41540001' in open(os.path.join(N.CSRC, 'mi_ode_rows_adjoint_t.h')).read()
    assert lib.mi_ode_adjoint_rows_t(None, None, None, None, None, None, None, None) == N.E_INVALID
    d, r = N.AdjointRowsTDesc(), N.Rhs()
    assert lib.mi_ode_adjoint_rows_t(C.byref(d), C.byref(r), None, None, None, None, None, None) == N.E_INVALID


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()[:16]


# sha256[:16] of the generated sources of the kinds that existed before this feature, computed on the commit before it: the plugin cache keys on them
PINNED = {
    'discrete_all': '65fc405bc7133472', 'rows_adjoint_all': '54570d4a9748c7a4',
    'lowered_rowlocal_f32': 'f3cef29084d60295', 'lowered_rowlocal_f64': 'c72025812dc31eb0',
    'lowered_rows_f32': '2d955c031f803f21', 'lowered_rows_f64': 'aff365472744fa8a',
    'vdp_hyper_f32': 'c5e406741b4deb0d', 'vdp_hyper_f64': '74c8ea359761697e',
    'vdp_rowlocal_f32': '1067f2b41a6e4b7b', 'vdp_rowlocal_f64': '41c207561bbdea68',
    'vdp_rows_f32': 'eeeb7bfc7211bbad', 'vdp_rows_f64': '5c5e3d89b3dc39fc',
}


def test_rows_t_source_is_a_kind_of_its_own_and_the_existing_kinds_hash_as_before():
    vdp = PC.van_der_pol()
    from tfdiffeq_amd import _plugin_build as PB
    from tfdiffeq_amd import lower
    for dt in PC.DTYPES:
        src, base = vdp.rows_t_source(dt), vdp.source(dt)
        assert '#include "mi_ode_rows_t_plugin.h"' in src and 'MI_ODE_DEFINE_ROWS_T_PLUGIN(mi::RhsUser)' in src
        assert 'mi_ode_plugin.h"' not in src and 'mi_ode_rows_plugin.h"' not in src and 'MI_ODE_DEFINE_ROWLOCAL_PLUGIN' not in src
        assert src.replace('mi_ode_rows_t_plugin.h', 'mi_ode_plugin.h').replace('MI_ODE_DEFINE_ROWS_T_PLUGIN(', 'MI_ODE_DEFINE_ROWLOCAL_PLUGIN(') == base
    roots = PB._source_roots(vdp.rows_t_source(F64))
    assert roots == ('mi_ode_rows_t_plugin.h',)
    hashed = [os.path.basename(p) for p in PB._plugin_headers(roots)]
    assert 'mi_ode_rows_t.h' in hashed and 'mi_ode_rows.h' in hashed and 'mi_ode_rows_core.h' in hashed
    for existing in (('mi_ode_plugin.h',), ('mi_ode_rows_plugin.h',), ('mi_ode_rows_adjoint_plugin.h',), ('mi_ode_hyper_plugin.h',), ('mi_ode_discrete_plugin.h',)):
        assert 'mi_ode_rows_t.h' not in [os.path.basename(p) for p in PB._plugin_headers(existing)]     # (no existing plugin is rebuilt)
    with pytest.raises(ValueError):
        rhs.rows_t_source_of(rhs.CustomCoop(40, "k = -y[i];").source(F64))
    a, b = RC.sources('cpu'), RC.sources('cpu')
    assert a == b and len(a) == 20 and sum('mi_ode_rows_t_plugin.h' in s for s in a) == 10 and sum('mi_ode_rows_adjoint_t_plugin.h' in s for s in a) == 4
    import per_trajectory_adjoint_cases as AC
    for mod, y0 in AC.modules('cpu'):
        base = lower.adjoint_source(lower.trace(mod, y0))
        src = rhs.rows_adjoint_t_source_of(base)
        assert src in a and '#include "mi_ode_rows_adjoint_t_plugin.h"' in src and 'MI_ODE_DEFINE_ROWS_ADJOINT_T_PLUGIN(mi::RhsUser)' in src
        assert 'mi_ode_rows_adjoint_plugin.h"' not in src and 'MI_ODE_DEFINE_ROWS_ADJOINT_PLUGIN' not in src
        assert src.replace('mi_ode_rows_adjoint_t_plugin.h', 'mi_ode_rows_adjoint_plugin.h').replace('_ADJOINT_T_PLUGIN(', '_ADJOINT_PLUGIN(') == base
        assert PB._source_roots(src) == ('mi_ode_rows_adjoint_t_plugin.h',)
    for existing in (('mi_ode_plugin.h',), ('mi_ode_rows_plugin.h',), ('mi_ode_rows_adjoint_plugin.h',), ('mi_ode_rows_t_plugin.h',)):
        assert 'mi_ode_rows_adjoint_t.h' not in [os.path.basename(p) for p in PB._plugin_headers(existing)]     # (no existing plugin is rebuilt)
    with pytest.raises(ValueError):
        rhs.rows_adjoint_t_source_of(vdp.source(F64))
    got = {}
    for k, dt in (('f64', torch.float64), ('f32', torch.float32)):
        low = lower.sources_for(PC.time_callable, torch.zeros(2, PC.TIME_DIM, dtype=dt))
        got.update({'vdp_rowlocal_' + k: _sha(vdp.source(dt)), 'vdp_rows_' + k: _sha(vdp.rows_source(dt)), 'vdp_hyper_' + k: _sha(vdp.hyper_source(dt)),
                    'lowered_rowlocal_' + k: _sha('\n'.join(low)), 'lowered_rows_' + k: _sha('\n'.join(rhs.rows_source_of(s) for s in low))})
    got['rows_adjoint_all'] = _sha('\n'.join(AC.adjoint_sources('cpu')))
    import discrete_lowered_cases as DC
    got['discrete_all'] = _sha('\n'.join(DC.discrete_sources('cpu')))
    assert got == PINNED, got
