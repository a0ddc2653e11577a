"""Fixed-grid solves and exact gradients on every row's own time grid, without a GPU: the refusals of `odeint` and `odeint.plan`, the pinned
options['per_trajectory'] refusal, valid inputs that reach the device check, the generated plugin sources, the C ABI's new entry points and
the forward walk (csrc/mi_ode_fixed_rows_t.h: fixed_rows_walk) compiled with g++ and held to the oracle's fixed-grid solve of every row."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_row_fixed_cases as FC                           # noqa: E402
import per_row_times_cases as RC                           # noqa: E402
import per_trajectory_cases as PC                          # noqa: E402
from oracle import ode_numpy as O                          # noqa: E402
from tests import bands, discrete_restatement as DR        # noqa: E402
from tests.test_gpu_per_trajectory import band64, f32_ceiling   # noqa: E402
from tfdiffeq_amd import _native as N, dispatch as D, lower, odeint, rhs   # noqa: E402

F64 = torch.float64
ROOT = FC.ROOT


def _t2(batch=6, T=5):
    return torch.as_tensor(RC.horizon_t(batch, T))


REFUSALS = [
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'midpoint', {}, 'no one-launch forward kernel'),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'heun', {}, 'no one-launch forward kernel'),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'explicit_adams', {}, 'no one-launch forward kernel'),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'rk4', {'step_size': 0.1}, "options['step_size']"),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'rk4', {'grid_constructor': lambda f, y, t: t}, "options['grid_constructor']"),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'euler', {'eps': 1e-3}, "options['eps']"),
    (rhs.Linear.from_matrix(torch.eye(4, dtype=F64)), torch.ones(6, 4, dtype=F64), _t2(), 'rk4', {}, 'matrix-core or cooperative'),
    (PC.time_callable, torch.ones(6, 4, dtype=F64), _t2(), 'rk4', {'lower': False}, "options['lower'] is False"),
    (rhs.Lorenz(), (torch.ones(6, 3, dtype=F64), torch.ones(6, 3, dtype=F64)), _t2(), 'rk4', {}, 'a tuple state'),
    (rhs.Lorenz(), torch.ones(2, 3, 3, dtype=F64), _t2(2), 'rk4', {}, 'a state of shape'),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(5), 'rk4', {}, '`t` of shape'),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'rk4', {'t_lengths': torch.ones(5, dtype=torch.int32)}, "options['t_lengths'] of shape"),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'rk4', {'t_lengths': torch.ones(6)}, 'must be an integer tensor'),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'rk4', {'process_group': object()}, 'a sharded run'),
    (rhs.MLP(torch.randn(8, 16, dtype=F64), torch.zeros(16, dtype=F64), torch.randn(16, 16, dtype=F64), torch.zeros(16, dtype=F64),
             torch.randn(16, 8, dtype=F64), torch.zeros(8, dtype=F64)), torch.ones(6, 8, dtype=F64), _t2(), 'rk4', {}, 'matrix-core or cooperative kernels (MLP'),
    (rhs.CustomCoop(40, "k = -y[i];", torch_fn=lambda t, y: -y), torch.ones(6, 40, dtype=F64), _t2(), 'euler', {},
     'matrix-core or cooperative kernels (CustomCoop, dim 40)'),
    (rhs.Conv2dODE(torch.zeros(4, 2, 1, 1, dtype=F64), torch.zeros(4, dtype=F64), torch.zeros(4, 4, 3, 3, dtype=F64), torch.zeros(4, dtype=F64),
                   torch.zeros(2, 4, 1, 1, dtype=F64), torch.zeros(2, dtype=F64)), torch.zeros(2, 2, 6, 6, dtype=F64), _t2(2), 'rk4', {},
     'matrix-core or cooperative kernels (Conv2dODE'),
    ((lambda t, y: torch.tanh(y) * 1.5), torch.ones(6, 40, dtype=F64), _t2(), 'rk4', {}, "a lowered 'coop' program, dim 40"),
    ((lambda t, y: y * float(y.sum())), torch.ones(6, 3, dtype=F64), _t2(), 'rk4', {}, 'the tracer refuses this callable'),
    (rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), 'adams', {}, 'no one-launch forward kernel'),
]


@pytest.mark.parametrize('case', range(len(REFUSALS)))
def test_refusals_from_odeint_and_plan(case):
    f, y0, t, method, opts, fragment = REFUSALS[case]
    with pytest.raises(ValueError) as e:
        odeint(f, y0, t, method=method, options=opts or None)
    assert fragment in str(e.value) and str(e.value).startswith(D.FIXED_ROWS_T_REFUSED), str(e.value)
    p = odeint.plan(f, y0, t, method=method, options=opts or None)
    assert p['engine'] == 'refused' and p['why'] == str(e.value), p


def test_values_are_refused_with_the_row():
    y = torch.ones(6, 3, dtype=F64)
    with pytest.raises(ValueError, match='must lie in 1 .. T'):
        odeint(rhs.Lorenz(), y, _t2(), method='rk4', options={'t_lengths': torch.tensor([1, 2, 3, 4, 5, 6])})
    mixed = _t2()
    mixed[2] = -mixed[2]
    with pytest.raises(ValueError, match='different directions'):
        odeint(rhs.Lorenz(), y, mixed, method='rk4')
    crooked = _t2()
    crooked[4, 3] = crooked[4, 2]
    with pytest.raises(AssertionError, match='row 4'):
        odeint(rhs.Lorenz(), y, crooked, method='euler')
    with pytest.raises(ValueError, match="needs a 2-D `t`"):
        odeint(rhs.Lorenz(), y, torch.linspace(0., 1., 5), method='rk4', options={'t_lengths': torch.ones(6, dtype=torch.int32)})


def test_per_trajectory_with_a_fixed_grid_method_stays_refused():
    for method in ('euler', 'rk4'):
        with pytest.raises(ValueError, match='every row already takes the same steps on a fixed grid'):
            odeint(rhs.Lorenz(), torch.ones(6, 3, dtype=F64), _t2(), method=method, options={'per_trajectory': True})


def test_valid_inputs_reach_the_device_check_and_plan_names_the_kernel():
    y3 = torch.ones(6, 3, dtype=F64)
    t, lengths = RC.ragged(6, T=4)
    for tt, opts in ((torch.as_tensor(t), {'t_lengths': torch.as_tensor(lengths)}), (-torch.as_tensor(t), {'t_lengths': torch.as_tensor(lengths).long()}),
                     (_t2(), None), (RC.horizon_t(6, 5).tolist(), None)):
        for method in FC.METHODS:
            with pytest.raises(N.NativeError):               # accepted (no ValueError): it is the device that is missing
                odeint(rhs.Lorenz(), y3, tt, method=method, options=opts)
            p = odeint.plan(rhs.Lorenz(), y3, tt, method=method, options=opts)
            assert p['engine'] == 'fused' and p['kernel'].startswith('k_fixed_rowlocal_t<double, %s>' % method) and p['launches'] == 'one per call', p
    p = odeint.plan(PC.time_callable, torch.ones(6, 4, dtype=torch.float32), _t2(), method='rk4')
    assert p['kernel'].startswith('k_fixed_rowlocal_t<float, rk4>') and p['lower']['lowered'], p
    assert 'k_fixed_rowlocal_t' not in str(odeint.plan(rhs.Lorenz(), y3, torch.linspace(0., 1., 5), method='rk4'))


def test_new_sources_differ_in_header_and_macro_only_and_the_abi_is_additive():
    src = PC.van_der_pol().source(F64)
    new = rhs.fixed_rows_t_source_of(src)
    assert new == src.replace('#include "mi_ode_plugin.h"', '#include "mi_ode_fixed_rows_t_plugin.h"').replace(
        'MI_ODE_DEFINE_ROWLOCAL_PLUGIN(', 'MI_ODE_DEFINE_FIXED_ROWS_T_PLUGIN(') and new != src
    f, _params, y0 = FC.DC.scalars('cpu', F64)
    dsrc = lower.discrete_source(lower.trace(f, y0))
    dnew = rhs.discrete_t_source_of(dsrc)
    assert dnew == dsrc.replace('#include "mi_ode_discrete_plugin.h"', '#include "mi_ode_discrete_t_plugin.h"').replace(
        'MI_ODE_DEFINE_DISCRETE_PLUGIN(', 'MI_ODE_DEFINE_DISCRETE_T_PLUGIN(') and dnew != dsrc
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    for name in ('mi_ode_integrate_fixed_rows_t', 'mi_ode_discrete_row_sweep_t'):
        assert name in N.EXPORTED_SYMBOLS and name + '(' in header
    assert N.ABI_VERSION == 13 and 'mi_ode_discrete_row_t_desc' in header


def test_library_entry_points_refuse_null_arguments():
    lib = N.load()
    assert lib.mi_ode_abi_version() == 13
    assert lib.mi_ode_integrate_fixed_rows_t(None, None, None, None, 0, None, None, None, None) == N.E_INVALID
    assert lib.mi_ode_discrete_row_sweep_t(None, None, None, None, None, None, None, None) == N.E_INVALID
    assert lib.mi_ode_discrete_row_t_sizeof() == C.sizeof(N.DiscreteRowTDesc)


@pytest.mark.parametrize('system', ['lorenz', 'lv'])
def test_host_walk_of_every_row_is_the_oracles_fixed_grid_solve(system, tmp_path):
    """fixed_rows_walk compiled by g++ (-ffp-contract=off) on RC.ragged(70, T=12) with NaN padding: every row against the oracle's solve on
    the row's own times - float64: |diff| <= 64 eps |ref|_max per row (both follow the same operation order; the bound leaves room for
    libm only; it lies inside band64) -, float32: the float instantiation on the float32-rounded inputs against the float64 oracle on those
    inputs, tests/bands.observed under f32_ceiling(steps, stages of the method) -, the padding exactly zero."""
    functor, dim, f_np = {'lorenz': (PC.LORENZ_FUNCTOR, 3, PC.lorenz_np), 'lv': (PC.LV_FUNCTOR, 2, PC.lv_np)}[system]
    inc = tmp_path / 'hip'
    inc.mkdir()
    (inc / 'hip_runtime.h').write_text('')
    src = tmp_path / 'walk.cpp'
    src.write_text(FC.host_walk_source(functor, dim))
    so = tmp_path / 'walk.so'
    cmd = ['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-I', str(tmp_path), '-I', os.path.join(ROOT, 'tfdiffeq_amd', 'csrc'),
           '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(so)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    lib = C.CDLL(str(so))
    t, lengths = RC.ragged(70, T=12, end=0.2)
    y0 = (PC.base_y0().numpy()[:, :dim] * (0.05 if system == 'lorenz' else 1.0)).copy()
    y0 = np.abs(y0) + 0.1 if system == 'lv' else y0
    scal = np.array([1.5, 1.0, 3.0, 1.0, 0, 0, 0, 0] if system == 'lv' else [10., 8. / 3., 28., 0, 0, 0, 0, 0], dtype=np.float64)
    for rk4, method in ((0, 'euler'), (1, 'rk4')):
        out = np.full((12, 70, dim), 7.0)
        lib.fixed_walk_f64(rk4, scal.ctypes.data_as(C.c_void_p), C.c_longlong(70), y0.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), 12,
                           lengths.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        for i in range(70):
            n = int(lengths[i])
            assert not out[n:, i].any()
            ref = O.odeint(f_np, y0[i:i + 1], t[i, :n], method=method)[:, 0] if n > 1 else y0[i:i + 1]
            assert np.max(np.abs(out[:n, i] - ref)) <= 64 * 2.0 ** -53 * max(np.max(np.abs(ref)), 1e-300), (system, method, i)
        y32, t32 = y0.astype(np.float32), np.where(np.isnan(t), np.nan, t.astype(np.float32).astype(np.float64))
        out32 = np.full((12, 70, dim), 7.0, dtype=np.float32)
        lib.fixed_walk_f32(rk4, scal.ctypes.data_as(C.c_void_p), C.c_longlong(70), y32.ctypes.data_as(C.c_void_p), t32.ctypes.data_as(C.c_void_p), 12,
                           lengths.ctypes.data_as(C.c_void_p), out32.ctypes.data_as(C.c_void_p))
        worst = 0.0
        for i in range(70):
            n = int(lengths[i])
            assert not out32[n:, i].any()
            ref = O.odeint(f_np, y32[i:i + 1].astype(np.float64), t32[i, :n], method=method)[:, 0] if n > 1 else y32[i:i + 1]
            obs, ceil = bands.observed(out32[:n, i], ref), f32_ceiling(max(n - 1, 1), 4 if rk4 else 1)
            worst = max(worst, obs)
            assert obs <= ceil, (system, method, i, obs, ceil)
        print('%s %s float32 walk: worst observed %.3e' % (system, method, worst))


# ---- a lowered callable: the forward walk and the masked reverse loop of a wavefront, g++ -------------------------------------------------
_LOWERED_LIBS = {}


def _lowered(name):
    """(library, trace, f, params, y0) of DC.<name> at batch 70 in float64: lower.host_vjp_source + FC.HOST_LOWERED_ENTRY."""
    if name not in _LOWERED_LIBS:
        from tests.test_discrete_lowered_host import _compile
        f, params, y0 = {'scalars': FC.DC.scalars, 'spiral': FC.DC.spiral, 'tanh8': FC.DC.tanh8}[name]('cpu', F64, 0, batch=70)
        tr = lower.trace(f, y0)
        _LOWERED_LIBS[name] = (_compile(FC.host_lowered_source(tr), 'per_row_fixed_' + name, extra=['-I', N.CSRC]), tr, f, params, y0)
    return _LOWERED_LIBS[name]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _per_row_reference(f, params, y0, t, lengths, method, w):
    """(solution [T, batch, dim] with NaN in the padding, grad y0, [parameter gradients summed over the rows]) of the float64 restatement,
    row by row on the row's own times."""
    T, batch = t.shape[1], y0.shape[0]
    sol = torch.full((T,) + tuple(y0.shape), float('nan'), dtype=F64)
    gy0, gps = torch.zeros_like(y0), [torch.zeros_like(p) for p in params]
    for i in range(batch):
        n = int(lengths[i])
        s_, gy, gp = DR.gradients(f, params, y0[i:i + 1], torch.as_tensor(t[i, :n]), method, w[:n, i:i + 1])
        sol[:n, i] = s_[0][:, 0]
        gy0[i] = gy[0][0]
        for acc, g in zip(gps, gp):
            if g is not None:
                acc += g
    return sol, gy0, gps


@pytest.mark.parametrize('name', FC.BACKWARD)
def test_host_walk_and_masked_sweep_of_a_lowered_callable(name):
    """On RC.ragged(70, 12) with NaN in the padding of `t`, of the stored solution and of the cotangent (none of it may be read).  Forward:
    fixed_rows_walk around the generated functor against the restatement's solve of every row (band64; float32 under f32_ceiling), padding
    exactly 0.  Backward: the loop of a wavefront of k_discrete_rowlocal_t - down from the wavefront's largest length, every lane every
    call, active mask, lam picked up at len - 1, len == 1 - over the unchanged discrete_row_step with a plain masked accumulator, against
    discrete_restatement.gradients per row (DC.rel under DR.ceiling64(T - 1, method)); rows of length 1 return their cotangent exactly;
    the number of discrete_row_step calls is 64 x (largest length - 1) per wavefront."""
    from tests.test_discrete_lowered_host import _pool, _tableau_arrays
    lib, tr, f, params, y0 = _lowered(name)
    lib.sweep_t_f64.restype = C.c_longlong
    dim = int(y0.shape[1])
    t, lengths = RC.ragged(70, T=12, end=FC.DC.t_end(name, F64))
    w = torch.randn((12,) + tuple(y0.shape), generator=torch.Generator().manual_seed(7), dtype=F64)
    pool, ps = _pool(tr)
    plist, P = lower.vjp_params(tr)
    pad = np.arange(12)[:, None] >= lengths[None, :]
    for method in FC.METHODS:
        sol, gy_ref, gp_ref = _per_row_reference(f, params, y0, t, lengths, method, w)
        # forward
        y_np = np.ascontiguousarray(y0.numpy())
        out = np.full((12, 70, dim), 7.0)
        lib.walk_t_f64(int(method == 'rk4'), ps, _ptr(pool), C.c_longlong(70), _ptr(y_np), _ptr(t), 12, _ptr(lengths), _ptr(out))
        assert not out[pad].any()
        band64(out[~pad], sol.numpy()[~pad], '%s %s host walk' % (name, method))
        y32, t32, pool32 = y_np.astype(np.float32), np.where(np.isnan(t), np.nan, t.astype(np.float32).astype(np.float64)), pool.astype(np.float32)
        out32 = np.full((12, 70, dim), 7.0, dtype=np.float32)
        lib.walk_t_f32(int(method == 'rk4'), ps, _ptr(pool32), C.c_longlong(70), _ptr(y32), _ptr(t32), 12, _ptr(lengths), _ptr(out32))
        assert not out32[pad].any()
        obs = bands.observed(out32[~pad], sol.numpy()[~pad])
        assert obs <= f32_ceiling(11, 4 if method == 'rk4' else 1), (name, method, obs)
        # backward: the stored solution and the cotangent carry NaN in the padding
        ys = np.ascontiguousarray(sol.numpy())
        gys = np.ascontiguousarray(torch.where(torch.as_tensor(pad)[:, :, None], torch.full_like(w, float('nan')), w).numpy())
        gy0, gth = np.zeros((70, dim)), np.zeros(max(P, 1))
        S, a, b, c = _tableau_arrays(method)
        calls = lib.sweep_t_f64(S, _ptr(a), _ptr(b), _ptr(c), 12, C.c_longlong(70), _ptr(t), _ptr(lengths), _ptr(ys), _ptr(gys), _ptr(gy0), _ptr(gth),
                                ps, _ptr(pool))
        assert calls == 64 * 11 + 64 * (int(lengths[64:].max()) - 1), calls      # two wavefronts: rows 0 .. 63 reach 12, rows 64 .. 69 reach 10
        assert np.isfinite(gy0).all() and np.isfinite(gth).all()
        for i in np.nonzero(lengths == 1)[0]:
            assert np.array_equal(gy0[i], w[0, i].numpy()), i
        ceil = DR.ceiling64(11, method)
        errs = [FC.DC.rel(torch.tensor(gy0), gy_ref)]
        for i, off, n in plist:
            k = [j for j, p in enumerate(params) if p is tr.tensors[i]['t']][0]
            errs.append(FC.DC.rel(torch.tensor(gth[off:off + n]).reshape(params[k].shape), gp_ref[k]))
        assert len(errs) == 1 + len(params)
        print(name, method, ['%.2e' % e for e in errs], 'ceiling %.2e' % ceil)
        assert max(errs) <= ceil, (name, method, errs, ceil)
