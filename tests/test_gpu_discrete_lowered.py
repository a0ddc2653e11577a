"""GPU tests of the fused row-local sweep of `odeint_discrete(..., lower=True)`: the whole backward of a lowered Python callable in one
launch (generated vjp, csrc/mi_ode_discrete_row.h), against autograd through the float64 CPU restatement of the same discrete map
(tests/discrete_restatement.py).

Metric, per gradient tensor: DR.rel_max = max|got - ref| / max|ref| (an exactly zero reference gradient asks for an exactly zero gradient:
discrete_lowered_cases.rel).  Ceilings: DR.ceiling64(n - 1, method) and DR.ceiling32(n - 1, method).  Every float32 case first asserts that
the float32 CPU restatement itself is inside the ceiling against its float64 twin."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discrete_lowered_cases as DC                       # noqa: E402
from tests import discrete_restatement as DR              # noqa: E402
from tfdiffeq_amd import discrete, odeint, odeint_discrete   # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
GRIDS = (('euler', 2), ('midpoint', 5), ('heun', 5), ('rk4', 2), ('rk4', 5), ('rk4', 21))
UNEVEN = (0., .1, .35, .4, 1.)
MAKERS = dict(DC.SYSTEMS, tanh8_1100=DC.tanh8_batch(1100), interleave_b=DC.interleave_b, transposed=DC.refused_transposed, tuple=DC.refused_tuple)


def _times(name, grid, dtype):
    """grid: a number of points (uniform on [0, T]) or a tuple of fractions of T; T = DC.t_end (the float32 spiral: [0, 0.5])."""
    T = DC.t_end(name, dtype) if name in DC.T_END else 1.0
    if isinstance(grid, int):
        return torch.linspace(0., T, grid, dtype=F64)
    return torch.tensor(grid, dtype=F64) * T


def _tup(x):
    return (x,) if isinstance(x, torch.Tensor) else tuple(x)


def _weights(y0, n, dtype=F64):
    g = torch.Generator().manual_seed(11)
    out = tuple(torch.randn((n,) + tuple(y.shape), generator=g, dtype=F64).to(dtype) for y in _tup(y0))
    return out[0] if isinstance(y0, torch.Tensor) else out


@functools.lru_cache(maxsize=None)
def reference64(name, method, grid, dtype=F64):
    """(solution, [y0 gradients + parameter gradients]) of the float64 CPU restatement on the grid of the `dtype` case - computed once per
    case, shared, never changed."""
    f, params, y0 = MAKERS[name]('cpu', F64)
    t = _times(name, grid, dtype)
    sol, gy, gp = DR.gradients(f, params, y0, t, method, _weights(y0, t.shape[0]))
    assert all(bool(torch.isfinite(g).all()) for g in gy + gp)
    return sol, gy + gp


def guard32(name, method, grid, ceil):
    f, params, y0 = MAKERS[name]('cpu', F32)
    t = _times(name, grid, F32)
    _, gy, gp = DR.gradients(f, params, y0, t, method, _weights(y0, t.shape[0], F32))
    worst = max(DC.rel(a, b) for a, b in zip(gy + gp, reference64(name, method, grid, F32)[1]))
    print('%s %s %s: float32 CPU restatement vs float64: %.3e (ceiling %.3e)' % (name, method, grid, worst, ceil))
    assert worst <= ceil, 'the float32 restatement itself is %.3e off its float64 twin (ceiling %.3e)' % (worst, ceil)


def run(name, method, grid, dtype, lower, made=None):
    f, params, y0 = made if made is not None else MAKERS[name]('cuda:0', dtype)
    t = _times(name, grid, dtype)
    ys = tuple(y.clone().requires_grad_(True) for y in _tup(y0))
    w = _weights(y0, t.shape[0], dtype)
    sol = odeint_discrete(f, ys[0] if isinstance(y0, torch.Tensor) else ys, t, method=method, lower=lower)
    loss = sum((w_.to('cuda:0') * s_).sum() for w_, s_ in zip(_tup(w), _tup(sol)))
    grads = torch.autograd.grad(loss, ys + tuple(params), allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, ys + tuple(params))]
    return [s_.detach() for s_ in _tup(sol)], grads, dict(odeint_discrete.last_backward_stats), (f, params, y0)


def compare(got, ref, ceil, what):
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.is_cuda
        err = DC.rel(a, b)
        worst = max(worst, err)
        print('%s tensor %d: %.3e (ceiling %.3e)' % (what, i, err, ceil))
    assert worst <= ceil, '%s: max|got - ref| / max|ref| = %.3e above the ceiling %.3e' % (what, worst, ceil)


def check_fused(name, method, grid, dtype):
    n = grid if isinstance(grid, int) else len(grid)
    ceil = DR.ceiling64(n - 1, method) if dtype == F64 else DR.ceiling32(n - 1, method)
    if dtype == F32:
        guard32(name, method, grid, ceil)
    sol, grads, stats, made = run(name, method, grid, dtype, True)
    assert stats['engine'] == 'fused row-local sweep' and stats['n_launches'] == 1 and stats['n_steps'] == n - 1 and stats['why'] == '', stats
    assert stats['n_params'] == sum(p.numel() for p in made[1])
    for g, x in zip(grads[1:], made[1]):
        assert g.shape == x.shape and g.dtype == x.dtype and g.device == x.device
    compare(grads, reference64(name, method, grid, dtype)[1], ceil, '%s %s %s %s' % (name, method, grid, dtype))
    with torch.no_grad():
        plain = odeint(made[0], made[2], _times(name, grid, dtype), method=method)
    assert torch.equal(sol[0], plain)
    sol2, grads2, _, _ = run(name, method, grid, dtype, True, made=made)
    assert torch.equal(sol[0], sol2[0]) and all(torch.equal(a, b) for a, b in zip(grads, grads2)), 'a second identical call differs'
    return grads


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('method,n', GRIDS)
@pytest.mark.parametrize('name', sorted(DC.SYSTEMS))
def test_fused_row_local_sweep(name, method, n, dtype):
    check_fused(name, method, n, dtype)


@pytest.mark.parametrize('name', sorted(DC.SYSTEMS))
def test_uneven_and_decreasing_grids(name):
    check_fused(name, 'rk4', UNEVEN, F64)
    check_fused(name, 'rk4', UNEVEN[::-1], F64)


@pytest.mark.parametrize('row_grid', [1, 2, 0])
def test_row_groups_ragged_wavefront_and_the_fold_over_workgroups(row_grid, monkeypatch):
    """Batch 1100 = 4 groups of 256 rows + 76: several row groups per workgroup (grid 1, 2), a last wavefront with 12 of 64 lanes, the fold
    over 1, 2 and 5 workgroups."""
    monkeypatch.setattr(discrete, 'ROW_GRID', row_grid)
    check_fused('tanh8_1100', 'rk4', 5, F64)
    check_fused('tanh8_1100', 'heun', 5, F32)


def test_interleaved_calls_keep_their_own_constants():
    """forward A, forward B, backward A, backward B - B is the same code (one program, one shared pool buffer) with other parameter values."""
    t = _times('scalars', 5, F64)
    sols, ys, made = [], [], []
    for name in ('scalars', 'interleave_b'):
        f, params, y0 = MAKERS[name]('cuda:0', F64)
        y = y0.clone().requires_grad_(True)
        sols.append(odeint_discrete(f, y, t, method='rk4', lower=True))
        ys.append(y)
        made.append((f, params, y0))
    for name, sol, y, (f, params, y0) in zip(('scalars', 'interleave_b'), sols, ys, made):
        w = _weights(y0, 5).to('cuda:0')
        grads = torch.autograd.grad((w * sol).sum(), (y,) + tuple(params))
        assert odeint_discrete.last_backward_stats['engine'] == 'fused row-local sweep'
        compare(grads, reference64(name, 'rk4', 5)[1], DR.ceiling64(4, 'rk4'), 'interleaved ' + name)


@pytest.mark.parametrize('name', ['transposed', 'tuple'])
def test_auto_falls_back_to_the_generic_sweep_and_says_why(name):
    _, grads, stats, _ = run(name, 'rk4', 5, F64, 'auto')
    assert stats['engine'] == 'generic sweep' and 'fused row-local sweep: ' in stats['why'] and len(stats['why']) > 30, stats
    compare(grads, reference64(name, 'rk4', 5)[1], DR.ceiling64(4, 'rk4'), 'auto ' + name)
    with pytest.raises(ValueError, match='fused row-local sweep does not take this call'):
        run(name, 'rk4', 5, F64, True)
