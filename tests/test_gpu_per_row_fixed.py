"""Fixed-grid solves and exact gradients on every row's own time grid, on the GPU (euler / rk4 with `t` [batch, T] and options['t_lengths'];
csrc/mi_ode_fixed_rows_t.h: k_fixed_rowlocal_t, csrc/mi_ode_discrete_row_t.h: k_discrete_rowlocal_t).

Forward: row i of a call is torch.equal to `odeint(func, y0[i:i+1], t[i, :len_i], method=m)[:, 0]` on the existing one-launch kernel, the
padding is exactly 0.  Backward: grad y0[i] is torch.equal to the batch-of-one `odeint_discrete(..., lower=True)`; all gradients against
the float64 CPU restatement (tests/discrete_restatement.gradients per row on the row's own times, the loss weights of
test_gpu_discrete_lowered._weights, the metric DC.rel) under the project's ceilings DR.ceiling64(T - 1, m) / DR.ceiling32(T - 1, m); every
float32 case first asserts that the float32 restatement itself is inside the ceiling.

The van_der_pol (dim 2) and time_callable (dim 4) states are PC.base_y0()'s columns scaled by 0.01 and 0.1, so that their rows stay finite on
these grids; rhs.Lorenz runs on PC.base_y0() itself.

Shapes.  Batch 70 (one full wavefront, one with 6 live lanes), T = 5 (RC.horizon_t) and the ragged T = 12 with lengths cycling through
1 .. 12 and NaN in the padding of `t`; batch 1100 for several workgroups, row groups per workgroup and the fold over workgroups.

The batch-of-one references ask for the lowered kernel explicitly (options={'lower': True}): tests/conftest.py switches the automatic
lowering off for this module, and a Python callable on the plane kernels is not the one-launch kernel the rows are defined against."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discrete_lowered_cases as DC                        # noqa: E402
import per_row_fixed_cases as FC                           # noqa: E402
import per_row_times_cases as RC                           # noqa: E402
import per_trajectory_cases as PC                          # noqa: E402
from tests import discrete_restatement as DR               # noqa: E402
from tests.test_gpu_discrete_lowered import _weights       # noqa: E402
from tfdiffeq_amd import discrete, odeint, odeint_discrete, rhs   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
ENGINE = "k_fixed_rowlocal_t: euler / rk4 on every row's own time grid (per-row times and lengths), one launch"
BWD_ENGINE = 'fused row-local sweep (per-row times)'
ONE_LAUNCH = {'lower': True}                                # the reference of every row: the existing one-launch kernels
FORWARD = {'lorenz': lambda: (rhs.Lorenz(), PC.base_y0()),
           'van_der_pol': lambda: (PC.van_der_pol(), PC.base_y0()[:, :2].contiguous() * 0.01),
           'time_callable': lambda: (PC.time_callable, torch.cat([PC.base_y0(), PC.base_y0()[:, :1]], dim=1) * 0.1)}


def same(a, b):
    """torch.equal, with NaN equal to NaN and nothing else loosened (an inf stays an inf): the stiffest Lorenz rows of PC.base_y0() (63, 64,
    69; 35 too in float32) overflow on the coarse grids of RC.horizon_t / RC.ragged, in the batch-of-one call exactly as in the row, so
    those rows test the definition on their finite points and the NaN pattern; test_forward_many_workgroups keeps every sampled row finite."""
    nan = torch.isnan(a)
    return a.shape == b.shape and torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan], b[~nan])


def fixed_call(f, y0, t, method, lengths=None):
    opts = None if lengths is None else {'t_lengths': torch.as_tensor(lengths)}
    sol = odeint(f, y0, torch.as_tensor(t), method=method, options=opts)
    st = dict(odeint.last_stats)
    assert st['engine'] == ENGINE and st['n_launches'] == 1 and st['route'] == 'fused_rows_t', st
    return sol


def assert_row_is_the_batch_one_call(sol, f, y0, i, t_row, method):
    n = len(t_row)
    assert not sol[n:, i].any(), (method, i)
    if n == 1:
        assert torch.equal(sol[0, i], y0[i])
        return
    ref = odeint(f, y0[i:i + 1], torch.as_tensor(np.asarray(t_row)), method=method, options=ONE_LAUNCH)
    assert odeint.last_stats['n_launches'] == 1 and odeint.last_stats['route'] == 'fused', odeint.last_stats
    assert same(sol[:n, i], ref[:, 0]), (method, i, float((sol[:n, i] - ref[:, 0]).abs().max()))


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('method', FC.METHODS)
@pytest.mark.parametrize('name', sorted(FORWARD))
def test_forward_rows_are_the_batch_one_calls_bit_for_bit(name, method, dtype):
    f, y0 = FORWARD[name]()
    y0 = y0.to(device=DEV, dtype=dtype)
    t = RC.horizon_t(70, 5)
    sol = fixed_call(f, y0, t, method)
    assert sol.shape == (5,) + tuple(y0.shape) and sol.dtype == dtype and torch.equal(sol[0], y0)
    for i in PC.BASE_ROWS:
        assert_row_is_the_batch_one_call(sol, f, y0, i, t[i], method)
    assert same(fixed_call(f, y0, t, method), sol)                                   # a second identical call: the same bits
    tr, lengths = RC.ragged(70, 12)
    sol = fixed_call(f, y0, tr, method, lengths)
    assert sol.shape == (12,) + tuple(y0.shape)
    for i in set(PC.BASE_ROWS) | {0, 1, 11, 12, 13, 23}:                                  # (lengths 1, 2 and T = 12 among them)
        assert_row_is_the_batch_one_call(sol, f, y0, i, tr[i, :lengths[i]], method)
    pad = torch.as_tensor(np.arange(12)[:, None] >= lengths[None, :], device=DEV)
    assert not sol[pad].any()
    # all rows decreasing: the mirrored result (the sign goes to the right-hand side once)
    back = fixed_call(f, y0, -tr, method, lengths)
    i = 23
    ref = odeint(f, y0[i:i + 1], torch.as_tensor(-tr[i, :lengths[i]]), method=method, options=ONE_LAUNCH)
    assert odeint.last_stats['n_launches'] == 1 and odeint.last_stats['route'] == 'fused', odeint.last_stats
    assert same(back[:lengths[i], i], ref[:, 0]) and not back[pad].any()


@pytest.mark.parametrize('dtype', [F64, F32])
def test_forward_many_workgroups(dtype):
    y0 = PC.base_y0().repeat(16, 1)[:1100].to(device=DEV, dtype=dtype)
    lengths = 1 + np.arange(1100) % 12
    t = FC.ragged_with(lengths, 12, end=0.02)                # (steps of at most 0.02 / 11: every row stays finite, so every bit is compared)
    sol = fixed_call(rhs.Lorenz(), y0, t, 'rk4', lengths.astype(np.int32))
    assert bool(torch.isfinite(sol).all())
    for i in (0, 255, 256, 700, 1023, 1024, 1099):
        assert_row_is_the_batch_one_call(sol, rhs.Lorenz(), y0, i, t[i, :lengths[i]], 'rk4')
    assert same(fixed_call(rhs.Lorenz(), y0, t, 'rk4', lengths.astype(np.int32)), sol)


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
def make(name, device, dtype, batch=70):
    return {'scalars': DC.scalars, 'spiral': DC.spiral, 'tanh8': DC.tanh8}[name](device, dtype, 0, batch=batch)


def row_times(kind, batch, end):
    """(t [batch, T], lengths [batch] | None)"""
    if kind == 'horizon':
        return RC.horizon_t(batch, 5, lo=0.5 * end, span=0.5 * end), None
    if kind == 'mixed':
        lengths = FC.mixed_lengths(batch, 12)
        return FC.ragged_with(lengths, 12, end), lengths
    return RC.ragged(batch, 12, end=end)


def per_row_restatement(name, method, kind, end, dtype, batch=70):
    """[grad y0 [batch, dim]] + [parameter gradients summed over the rows] of the CPU restatement in `dtype`, row by row on the row's times."""
    f, params, y0 = make(name, 'cpu', dtype, batch)
    t, lengths = row_times(kind, batch, end)
    T = t.shape[1]
    w = _weights(y0, T, dtype)
    gy0 = torch.zeros_like(y0)
    gps = [torch.zeros_like(p) for p in params]
    for i in range(batch):
        n = T if lengths is None else int(lengths[i])
        _, gy, gp = DR.gradients(f, params, y0[i:i + 1], torch.as_tensor(t[i, :n]), method, w[:n, i:i + 1])
        gy0[i] = gy[0][0]
        for acc, g in zip(gps, gp):
            if g is not None:
                acc += g
    out = [gy0] + gps
    assert all(bool(torch.isfinite(g).all()) for g in out)
    return out


@functools.lru_cache(maxsize=None)
def reference64(name, method, kind, end):
    return per_row_restatement(name, method, kind, end, F64)


def run(name, method, kind, dtype, batch=70, lower=None, poison=False, made=None, times=None):
    f, params, y0 = made if made is not None else make(name, DEV, dtype, batch)
    t, lengths = times if times is not None else row_times(kind, batch, DC.t_end(name, dtype))
    T = t.shape[1]
    y = y0.clone().requires_grad_(True)
    opts = None if lengths is None else {'t_lengths': torch.as_tensor(lengths)}
    sol = odeint_discrete(f, y, torch.as_tensor(t), method=method, options=opts, lower=lower)
    w = _weights(y0, T, dtype).to(DEV)
    if poison:                                               # the cotangent of the padding is never read
        w = w.clone()
        w[torch.as_tensor(np.arange(T)[:, None] >= np.asarray(lengths)[None, :], device=DEV)] = float('nan')
        grads = torch.autograd.grad(sol, (y,) + tuple(params), grad_outputs=w, allow_unused=True)
    else:
        grads = torch.autograd.grad((w * sol).sum(), (y,) + tuple(params), allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, (y,) + tuple(params))]
    st = dict(odeint_discrete.last_backward_stats)
    n_max = T if lengths is None else int(np.max(lengths))
    assert st['engine'] == BWD_ENGINE and st['n_launches'] == 1 and st['n_steps'] == n_max - 1 and st['why'] == '', st
    assert st['n_params'] == sum(p.numel() for p in params)
    return sol.detach(), grads, (f, params, y0), (t, lengths)


def assert_grad_y0_rows_are_the_batch_one_sweeps(grads, made, times, method, rows, dtype):
    f, params, y0 = made
    t, lengths = times
    T = t.shape[1]
    w = _weights(y0, T, dtype).to(DEV)
    for i in rows:
        n = T if lengths is None else int(lengths[i])
        if n == 1:
            assert torch.equal(grads[0][i], w[0, i]), i
            continue
        y = y0[i:i + 1].clone().requires_grad_(True)
        sol = odeint_discrete(f, y, torch.as_tensor(t[i, :n]), method=method, options=ONE_LAUNCH, lower=True)
        g, = torch.autograd.grad(sol, (y,), grad_outputs=w[:n, i:i + 1])
        assert odeint_discrete.last_backward_stats['engine'] == 'fused row-local sweep'
        assert odeint_discrete.last_backward_stats['forward'].get('n_launches') == 1, odeint_discrete.last_backward_stats
        assert torch.equal(grads[0][i], g[0]), (method, i, float((grads[0][i] - g[0]).abs().max()))


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('kind', ['ragged', 'horizon'])
@pytest.mark.parametrize('method', FC.METHODS)
@pytest.mark.parametrize('name', FC.BACKWARD)
def test_backward_rows_and_restatement(name, method, kind, dtype):
    end = DC.t_end(name, dtype)
    T = 12 if kind == 'ragged' else 5
    ceil = DR.ceiling64(T - 1, method) if dtype == F64 else DR.ceiling32(T - 1, method)
    ref = reference64(name, method, kind, end)
    if dtype == F32:
        worst = max(DC.rel(a, b) for a, b in zip(per_row_restatement(name, method, kind, end, F32), ref))
        print('%s %s %s: float32 CPU restatement vs float64: %.3e (ceiling %.3e)' % (name, method, kind, worst, ceil))
        assert worst <= ceil, 'the float32 restatement itself is %.3e off its float64 twin (ceiling %.3e)' % (worst, ceil)
    sol, grads, made, times = run(name, method, kind, dtype)
    # the forward is the fixed_rows solve, with the same values
    with torch.no_grad():                                    # (plain odeint refuses inputs that require grad on this route)
        assert torch.equal(sol, fixed_call(made[0], made[2], times[0], method, times[1]))
    assert_grad_y0_rows_are_the_batch_one_sweeps(grads, made, times, method, PC.BASE_ROWS + (12, 13, 23), dtype)       # (a)
    worst = 0.0                                                                                                          # (b)
    for k, (a, b) in enumerate(zip(grads, ref)):
        assert a.shape == b.shape and a.is_cuda and a.dtype == dtype
        err = DC.rel(a, b)
        worst = max(worst, err)
        print('%s %s %s %s tensor %d: %.3e (ceiling %.3e)' % (name, method, kind, dtype, k, err, ceil))
    assert worst <= ceil, 'max|got - ref| / max|ref| = %.3e above the ceiling %.3e' % (worst, ceil)
    if kind == 'ragged':                                                                                                 # (d)
        _, poisoned, _, _ = run(name, method, kind, dtype, poison=True)
        assert all(bool(torch.isfinite(g).all()) and torch.equal(g, h) for g, h in zip(poisoned, grads))


@pytest.mark.parametrize('dtype', [F64, F32])
def test_backward_reruns_are_bit_identical_on_every_grid(dtype):                                                         # (c)
    made = DC.tanh8_batch(1100)(DEV, dtype)
    times = RC.ragged(1100, 12, end=DC.t_end('tanh8', dtype))
    first = None
    try:
        for grid in (1, 2, 0):
            discrete.ROW_GRID = grid
            a = run('tanh8', 'rk4', 'ragged', dtype, made=made, times=times)[1]
            b = run('tanh8', 'rk4', 'ragged', dtype, made=made, times=times)[1]
            assert all(torch.equal(x, y) for x, y in zip(a, b)), grid
            if first is None:
                first = a
            assert torch.equal(a[0], first[0])               # grad y0 does not depend on the grid (the parameter sums' order does)
    finally:
        discrete.ROW_GRID = 0
    assert_grad_y0_rows_are_the_batch_one_sweeps(first, made, times, 'rk4', (0, 255, 256, 1023, 1024, 1099), dtype)


@pytest.mark.parametrize('method', FC.METHODS)
def test_backward_rows_of_length_one_and_mixed_wavefronts(method):
    made = make('scalars', DEV, F64)
    t = np.full((70, 12), np.nan)                                                                                        # (e)
    t[:, 0] = np.linspace(0., 1., 70)
    sol, grads, _, _ = run('scalars', method, None, F64, made=made, times=(t, np.ones(70, dtype=np.int32)))
    assert torch.equal(grads[0], _weights(made[2], 12, F64).to(DEV)[0]) and all(not g.any() for g in grads[1:])
    _, grads, made, times = run('scalars', method, 'mixed', F64)                                                         # (f)
    assert_grad_y0_rows_are_the_batch_one_sweeps(grads, made, times, method, tuple(range(0, 12)) + (62, 63, 64, 65, 66, 69), F64)
    ref = per_row_restatement('scalars', method, 'mixed', DC.t_end('scalars', F64), F64)
    assert max(DC.rel(a, b) for a, b in zip(grads, ref)) <= DR.ceiling64(11, method)


def test_refusals_at_the_call():
    f, params, y0 = make('scalars', DEV, F64)
    t, lengths = RC.ragged(70, 12)
    opts = {'t_lengths': torch.as_tensor(lengths)}
    with pytest.raises(ValueError, match='lower=False'):
        odeint_discrete(f, y0.clone().requires_grad_(True), torch.as_tensor(t), method='rk4', options=opts, lower=False)
    for key in ('linear', 'mlp64'):
        with pytest.raises(ValueError, match=r'odeint_discrete\(%s=True\): a 2-D `t`' % key):
            odeint_discrete(f, y0.clone().requires_grad_(True), torch.as_tensor(t), method='rk4', options=opts, **{key: True})
    for name, fragment in (('demo_net', 'a state of shape'), ('lorenz', 'a state of shape')):      # other state shapes
        g, _, z0 = DC.SYSTEMS[name](DEV, F64)
        with pytest.raises(ValueError, match=fragment):
            odeint_discrete(g, z0.clone().requires_grad_(True), torch.as_tensor(RC.horizon_t(int(z0.shape[0]), 5)), method='rk4')
