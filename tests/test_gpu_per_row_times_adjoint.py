"""Gradients of per-trajectory solves with per-row output times, lengths and tolerances on the MI355X: odeint_adjoint(module, y0, t [batch, T],
..., options={'per_trajectory': True, 't_lengths': ..}) - the forward on k_rows_rowlocal_t, the whole backward of every row in one launch
of k_rows_adjoint_t (csrc/mi_ode_rows_adjoint_t.h).

The definition: row i of the backward is the existing per-trajectory adjoint (k_rows_adjoint) on (y0[i:i+1], t[i, :len_i])
alone.  So grad y0[i], last_backward_stats['rows']['grad_params'][i], ['time_vjps'][i, :len_i] and the per-interval counts are torch.equal
to that batch-of-one call on the 1-D truncated row; the padding of time_vjps, of the counts and of grad t is exactly 0; grad theta is the
fixed-order sum of the rows (a workgroup's rows in row order, the workgroups in order) and a rerun gives the same bits.  Shapes: batch 70
(a full wavefront, one with six live lanes, dead lanes), 9 (a system that reads t) and 300 (two workgroups: the fold across them), T = 5 /
4 with lengths that cycle through 1 .. T and NaN in the padding of t."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_row_times_cases as RC                          # noqa: E402
import per_trajectory_adjoint_cases as AC                 # noqa: E402
import per_trajectory_cases as PC                         # noqa: E402
from tfdiffeq_amd import odeint_adjoint                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
TOL = {F64: dict(rtol=1e-6, atol=1e-9), F32: dict(rtol=1e-4, atol=1e-6)}
ENGINE_T = 'k_rows_adjoint_t: per-trajectory adjoint over per-row times, lengths or tolerances: every row its own augmented solve, one launch'
ENGINE_1 = 'k_rows_adjoint: per-trajectory adjoint: every row its own augmented solve with per-component control, one launch'
COUNTS = ('n_attempts', 'n_accepted', 'nfe')


def weights(n_t, row_ids, dim, dtype):
    """tests/test_gpu_per_trajectory_adjoint.py's: the loss is sum(sin(solution) * weights), weights that belong to the ROW and to the
    output index, so that a batch-of-one call on a truncated row sees the cotangent the batch call gave that row's first len_i outputs."""
    k = torch.arange(n_t * dim, dtype=F64).reshape(n_t, 1, dim)
    r = torch.as_tensor(list(row_ids), dtype=F64).reshape(1, -1, 1)
    return torch.cos(0.37 * k + 0.61 * r).to(device=DEV, dtype=dtype)


def call(mod, y_all, rows, t, dtype, method, lengths=None, engine=ENGINE_T, **kw):
    """One training step on the rows `rows` of y_all with the times `t` ([len(rows), T] or 1-D): every output on the device."""
    for p in mod.parameters():
        p.grad = None
    y0 = y_all[list(rows)].to(device=DEV, dtype=dtype).requires_grad_(True)
    tt = torch.tensor(np.asarray(t), dtype=F64, requires_grad=True)
    opts = dict(AC.ON) if lengths is None else dict(AC.ON, t_lengths=torch.as_tensor(np.asarray(lengths)))
    sol = odeint_adjoint(mod, y0, tt, method=method, options=opts, **dict(TOL[dtype], **kw))
    w = weights(sol.shape[0], rows, sol.shape[2], dtype)
    (torch.sin(sol) * w).sum().backward()                      # (cos(0) * w in the padding of a short row: a cotangent that must be ignored)
    st = dict(odeint_adjoint.last_backward_stats)
    assert st['engine'] == engine and st['n_launches'] == 1 and st['per_trajectory'] is True, st
    assert st['forward']['engine'].startswith('k_rows_rowlocal_t' if engine == ENGINE_T else 'k_rows_rowlocal:') and st['forward']['n_launches'] == 1
    assert not bool(st['rows']['status'].any())
    return dict(sol=sol.detach(), gy0=y0.grad.clone(), gp=torch.cat([p.grad.reshape(-1) for p in mod.parameters()]).clone(),
                gt=tt.grad.clone().to(DEV), rows=st['rows'], st=st)


def fixed_order_sum(x):
    """The kernel's fold of [batch, P]: the rows of a 256-row workgroup in row order, then the workgroups in order, in the state dtype."""
    groups = []
    for first in range(0, x.shape[0], 256):
        s = torch.zeros_like(x[0])
        for r in range(first, min(first + 256, x.shape[0])):
            s = s + x[r]
        groups.append(s)
    tot = torch.zeros_like(x[0])
    for s in groups:
        tot = tot + s
    return tot


def hold_rows_to_batch_of_one(name, dtype, method, y_all, t, lengths, check, **kw):
    mod = AC.SYSTEMS[name][0](dtype, DEV)
    B, T = t.shape
    full = call(mod, y_all, range(B), t, dtype, method, lengths, **kw)
    P = sum(p.numel() for p in mod.parameters())
    r = full['rows']
    assert full['sol'].shape == (T, B, 3) and full['gt'].shape == (B, T) and r['grad_params'].shape == (B, P) and r['time_vjps'].shape == (B, T)
    assert all(r[k].shape == (B, T - 1) for k in COUNTS)
    for i in check:
        n = int(lengths[i])
        one_kw = {k: (float(v[i]) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        one = call(mod, y_all, [i], t[i, :n], dtype, method, engine=ENGINE_1, **one_kw)         # the existing route on the truncated row, 1-D t
        assert torch.equal(full['sol'][:n, i], one['sol'][:, 0]) and not bool(full['sol'][n:, i].any()), i
        assert torch.equal(full['gy0'][i], one['gy0'][0]), (i, n, full['gy0'][i], one['gy0'][0])
        assert torch.equal(r['grad_params'][i], one['rows']['grad_params'][0]), (i, n)
        assert torch.equal(r['time_vjps'][i, :n], one['rows']['time_vjps'][0]) and not bool(r['time_vjps'][i, n:].any()), (i, n)
        for k in COUNTS:
            assert torch.equal(r[k][i, :n - 1], one['rows'][k][0]) and not bool(r[k][i, n - 1:].any()), (k, i, n, r[k][i], one['rows'][k][0])
        assert torch.equal(full['gt'][i, :n], one['gt']) and not bool(full['gt'][i, n:].any()), (i, n)
    # grad t is the rows' own time vjps, not summed; grad theta the fixed-order sum of the rows; a rerun has the same bits
    assert torch.equal(full['gt'], r['time_vjps'].to(F64))
    assert torch.equal(full['gp'], fixed_order_sum(r['grad_params'])), (full['gp'], fixed_order_sum(r['grad_params']))
    again = call(mod, y_all, range(B), t, dtype, method, lengths, **kw)
    for k in ('sol', 'gy0', 'gp', 'gt'):
        assert torch.equal(full[k], again[k]), k
    for k in ('grad_params', 'time_vjps') + COUNTS:
        assert torch.equal(r[k], again['rows'][k]), k
    return full


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('method', AC.METHODS)
def test_ragged_rows_are_the_batch_of_one_adjoints_bit_for_bit(method, dtype):
    """Lorenz, 70 rows, T = 5, lengths 5, 1, 2, 3, 4, 5, ..: the rows held are PC.BASE_ROWS (lengths 5, 5, 5, 3, 4, 4) and rows 1, 2 (lengths 1, 2)."""
    t, lengths = RC.ragged_adjoint_t('lorenz', 70)
    assert np.isnan(t).any() and sorted(set(lengths.tolist())) == [1, 2, 3, 4, 5]
    full = hold_rows_to_batch_of_one('lorenz', dtype, method, PC.base_y0(), t, lengths, sorted(set(PC.BASE_ROWS) | {1, 2}))
    att = full['rows']['n_attempts'].sum(dim=1)
    assert int(att[torch.as_tensor(lengths, device=DEV) == 1].max()) == 0 and int(att.max()) > 0       # a row of one time integrates nothing


@pytest.mark.parametrize('dtype', [F64, F32])
def test_a_module_that_reads_t_with_per_row_adjoint_tolerances(dtype):
    """TimeModule (its right-hand side and its vjp read t: a wrong per-row time shows), 9 rows, T = 4, ragged - with adjoint_rtol /
    adjoint_atol of every row's own: the row is the batch-of-one call at float(adjoint_rtol[i]), float(adjoint_atol[i])."""
    t, lengths = RC.ragged_adjoint_t('time', 9, T=4)
    art = torch.tensor(10.0 ** np.linspace(-3, -7, 9))
    hold_rows_to_batch_of_one('time', dtype, 'dopri5', AC.time_y0(), t, lengths, range(9), adjoint_rtol=art, adjoint_atol=art * 1e-2)


def test_two_workgroups_fold_in_a_fixed_order():
    """300 rows: the ticket fold across two workgroups (256 + 44 rows), equal to the ordered sum and identical on a rerun."""
    y_all = torch.cat([PC.base_y0()] * 5)[:300] * torch.linspace(0.5, 1.0, 300, dtype=F64)[:, None]
    t, lengths = RC.ragged_adjoint_t('lorenz', 300)
    hold_rows_to_batch_of_one('lorenz', F64, 'dopri5', y_all, t, lengths, (0, 255, 256, 299))


def test_shared_times_with_per_row_tolerances_sum_the_time_gradient():
    """A 1-D `t` with [batch] rtol routes to the new kernels too: grad t keeps the shape of t and is the sum of the rows' time vjps."""
    mod = AC.LorenzModule(F64, DEV)
    rtol = torch.tensor(10.0 ** np.linspace(-4, -7, 70))
    c = call(mod, PC.base_y0(), range(70), PC.BASE_T, F64, 'dopri5', rtol=rtol, atol=1e-9)
    assert c['gt'].shape == (5,) and torch.equal(c['gt'], c['rows']['time_vjps'].sum(dim=0))
    for i in (0, 69):
        one = call(mod, PC.base_y0(), [i], PC.BASE_T, F64, 'dopri5', engine=ENGINE_1, rtol=float(rtol[i]), atol=1e-9)
        assert torch.equal(c['gy0'][i], one['gy0'][0]) and torch.equal(c['rows']['time_vjps'][i], one['rows']['time_vjps'][0])
        assert all(torch.equal(c['rows'][k][i], one['rows'][k][0]) for k in COUNTS)
