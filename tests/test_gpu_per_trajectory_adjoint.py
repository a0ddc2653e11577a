"""Gradients for per-trajectory solves on the MI355X: odeint_adjoint(..., options={'per_trajectory': True}) - the forward on k_rows_rowlocal,
the whole backward of every row in one launch of k_rows_adjoint (csrc/mi_ode_rows_adjoint.h).

The definition everything is held to: row i of the backward is the reference's adjoint algorithm applied to trajectory i alone, started from
the stored forward output.  So (1) a row of a batch call equals the call on y0[i:i+1] in every bit, (2) every row agrees with the oracle's
AdaptiveRK on that row's four-component tuple (oracle.ode_numpy, fed the solution and the cotangent the device call itself saw) - counts
exactly in float64 -, (3) the summed gradients are the sums of the per-row outputs, (4) the existing route (odeint_adjoint without the
option on one row: the same algorithm with autograd vjps) agrees.  Shapes: batch 1, 70 (a full wavefront, one with six live lanes, dead
lanes), 257 (two workgroups: the cross-workgroup fold and its ticket); T = 2, 3, 4, 5."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_trajectory_adjoint_cases as AC                 # noqa: E402
import per_trajectory_cases as PC                         # noqa: E402
from tests.bands import observed                          # noqa: E402
from tfdiffeq_amd import odeint_adjoint                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
TOL = {F64: dict(rtol=1e-6, atol=1e-9), F32: dict(rtol=1e-4, atol=1e-6)}
ENGINE = 'k_rows_adjoint: per-trajectory adjoint: every row its own augmented solve with per-component control, one launch'
ROW_KEYS = ('grad_params', 'time_vjps', 'n_attempts', 'n_accepted', 'nfe', 'status')


def weights(n_t, row_ids, dim, dtype):
    """The loss is sum(sin(solution) * weights): weights that belong to the ROW (its index in the full batch), so that a sliced call sees
    the cotangent the batch call gave that row."""
    k = torch.arange(n_t * dim, dtype=F64).reshape(n_t, 1, dim)
    r = torch.as_tensor(list(row_ids), dtype=F64).reshape(1, -1, 1)
    return torch.cos(0.37 * k + 0.61 * r).to(device=DEV, dtype=dtype)


def adjoint_call(name, dtype, rows=None, t=None, method='dopri5', every=True, tol=None, mod=None, y0_all=None, **adjoint_kw):
    """One training step: (solution, cotangent, y0.grad, parameter grads in module order, t.grad, last_backward_stats, the module) - all on the device."""
    cls, _theta, _f, _aug, make_y0, t_default = AC.SYSTEMS[name]
    mod = cls(dtype, DEV) if mod is None else mod
    for p in mod.parameters():
        p.grad = None
    y_all = make_y0() if y0_all is None else y0_all
    rows = list(range(y_all.shape[0])) if rows is None else list(rows)
    y0 = y_all[rows].to(device=DEV, dtype=dtype).requires_grad_(True)
    tt = torch.tensor(np.asarray(t_default if t is None else t), dtype=F64, requires_grad=True)
    sol = odeint_adjoint(mod, y0, tt, method=method, options=AC.ON, **dict(tol or TOL[dtype], **adjoint_kw))
    seen = []
    sol.register_hook(lambda g_: seen.append(g_.detach().clone()))
    w = weights(sol.shape[0], rows, sol.shape[2], dtype)
    loss = (torch.sin(sol) * w).sum() if every else (torch.sin(sol[-1]) * w[-1]).sum()
    loss.backward()
    st = dict(odeint_adjoint.last_backward_stats)
    assert st['engine'] == ENGINE and st['n_launches'] == 1 and st['per_trajectory'] is True, st
    r = st['rows']
    B, T, P = len(rows), sol.shape[0], sum(p.numel() for p in mod.parameters())
    assert r['grad_params'].shape == (B, P) and r['time_vjps'].shape == (B, T) and r['status'].shape == (B,) and not bool(r['status'].any())
    assert all(r[k].shape == (B, T - 1) and r[k].is_cuda for k in ('n_attempts', 'n_accepted', 'nfe'))
    assert all(st[k] == int(r[k].sum(dim=1).max()) for k in ('n_attempts', 'n_accepted', 'nfe'))       # the maxima over rows
    assert st['forward']['engine'].startswith('k_rows_rowlocal') and st['forward']['n_launches'] == 1, st['forward']
    return dict(sol=sol.detach(), g=seen[0], gy0=y0.grad.clone(), gp=torch.cat([p.grad.reshape(-1) for p in mod.parameters()]).clone(), gt=tt.grad.clone().to(DEV),
                st=st, mod=mod)


def same_row(a, i, b, j):
    """Row i of call a and row j of call b: every per-row output, bit for bit."""
    assert torch.equal(a['sol'][:, i], b['sol'][:, j]) and torch.equal(a['gy0'][i], b['gy0'][j]), (i, j)
    for k in ROW_KEYS:
        assert torch.equal(a['st']['rows'][k][i], b['st']['rows'][k][j]), (k, i, j, a['st']['rows'][k][i], b['st']['rows'][k][j])


def band64(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = np.abs(got - ref) > 1e-6 + 1e-5 * np.abs(ref)
    assert not bad.any(), '%s: %d/%d outside band, max abs diff %.3e' % (what, bad.sum(), bad.size, np.abs(got - ref).max())


def oracle_row(name, c, i, dtype, tol, method='dopri5', t=None):
    """The oracle on row i of call c, from the solution and the cotangent the device call saw, in `dtype` (numpy)."""
    theta = AC.SYSTEMS[name][1](c['mod'])
    t = np.asarray(AC.SYSTEMS[name][5] if t is None else t, dtype=np.float64)
    ans, g = (x[:, i].cpu().numpy().astype(dtype) for x in (c['sol'], c['g']))
    return AC.oracle_backward(name, theta, t, ans, g, tol['rtol'], tol['atol'], method)


def row_np(c, i):
    r = c['st']['rows']
    return (c['gy0'][i].cpu().numpy(), r['grad_params'][i].cpu().numpy(), r['time_vjps'][i].cpu().numpy(),
            r['n_attempts'][i].tolist(), r['n_accepted'][i].tolist(), r['nfe'][i].tolist())


# ---- the row definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32])
def test_rows_are_the_batch_one_calls_bit_for_bit(dtype):
    full = adjoint_call('lorenz', dtype)                     # 70 rows, T = 5
    assert full['sol'].shape == (5, 70, 3) and full['gy0'].shape == (70, 3) and full['gp'].shape == (3,) and full['gt'].shape == (5,)
    for i in PC.BASE_ROWS:
        one = adjoint_call('lorenz', dtype, rows=[i])        # batch 1
        same_row(full, i, one, 0)
        assert torch.equal(one['gp'], one['st']['rows']['grad_params'][0]) and torch.equal(one['gt'], one['st']['rows']['time_vjps'][0].to(F64))
    part = adjoint_call('lorenz', dtype, rows=range(60, 70))  # re-slicing the batch changes nothing
    for i in (63, 64, 69):
        same_row(full, i, part, i - 60)
    again = adjoint_call('lorenz', dtype)                    # reruns are bit-identical, the summed gradients included
    for i in range(70):
        same_row(full, i, again, i)
    assert torch.equal(full['gp'], again['gp']) and torch.equal(full['gt'], again['gt']) and torch.equal(full['gy0'], again['gy0'])
    att = full['st']['rows']['n_attempts'].sum(dim=1)
    assert int(att.min()) < int(att.max())                   # the rows genuinely take different step sequences


# ---- against the oracle, row by row ---------------------------------------------------------------------------------------------------------
def test_rows_against_the_oracle_float64():
    """Counts exactly (attempts, accepted steps, function evaluations of every interval), values inside the float64 band."""
    c = adjoint_call('lorenz', F64)
    for i in PC.BASE_ROWS:
        got, ref = row_np(c, i), oracle_row('lorenz', c, i, np.float64, TOL[F64])
        assert got[3:] == tuple(ref[3:]), (i, got[3:], ref[3:])
        for a, b, what in zip(got[:3], ref[:3], ('grad_y0', 'grad_params', 'time_vjps')):
            band64(a, b, 'lorenz row %d %s' % (i, what))


def test_rows_against_the_oracle_float32():
    """Counts within max(2, attempts // 20) per interval.  The value ceiling is measured, reference against reference: the oracle in
    float32 and in float64 on the same rows, from the same solution and cotangent; the kernel gets 4 x the worst bands.observed deviation
    of the two (its FMA contraction and vjp summation order make its float32 rounding path a different one of the same size), never below
    the 2e-4 floor of f32_ceiling, never above the 1e-2 tests/bands.py grants gradient comparisons.  Measured on the CPU for the six
    BASE_ROWS (float32 oracle forward, rtol 1e-4 / atol 1e-6): worst float32-vs-float64 oracle deviation 1.6e-5 (row 0, grad_params), 4 x
    that is 6.3e-5, so the ceiling is the 2e-4 floor; the two oracles take the same attempts in every interval.  From the device's own
    float32 solution (what this test feeds them) the figure is 2.4e-5: the same ceiling.  The kernel is compared with the float32 oracle
    (observed on the MI355X: at most 2.6e-5, row 0, grad_params)."""
    c = adjoint_call('lorenz', F32)
    worst, pairs = 0.0, []
    for i in PC.BASE_ROWS:
        r32, r64 = oracle_row('lorenz', c, i, np.float32, TOL[F32]), oracle_row('lorenz', c, i, np.float64, TOL[F32])
        worst = max([worst] + [observed(a, b) for a, b in zip(r32[:3], r64[:3])])
        pairs.append((i, row_np(c, i), r32))
    ceiling = min(1e-2, max(2e-4, 4 * worst))
    print('float32 oracle against float64 oracle: worst observed %.3e -> ceiling %.3e' % (worst, ceiling))
    for i, got, ref in pairs:
        for k in range(len(ref[3])):
            assert abs(got[3][k] - ref[3][k]) <= max(2, ref[3][k] // 20), (i, k, got[3], ref[3])
        for a, b, what in zip(got[:3], ref[:3], ('grad_y0', 'grad_params', 'time_vjps')):
            obs = observed(a, b)
            print('row %d %s: observed %.3e' % (i, what, obs))
            assert obs <= ceiling, (i, what, obs, ceiling)


# ---- the sums, and where the gradients land ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32])
def test_sums_over_two_workgroups_and_where_the_gradients_land(dtype):
    """Batch 257: two workgroups, the second with one live lane - the fold of the workgroups' rows by the last one to arrive."""
    base = PC.base_y0()
    y_all = torch.cat([base, base * 0.7, base * 1.3, base[:47] * 0.4])
    assert y_all.shape[0] == 257
    t = PC.BASE_T[:3]
    c = adjoint_call('lorenz', dtype, t=t, y0_all=y_all)
    r, eps = c['st']['rows'], float(torch.finfo(dtype).eps)
    for got, terms in ((c['gp'], r['grad_params']), (c['gt'].to(dtype), r['time_vjps'])):
        ref = terms.to(F64).sum(dim=0)
        bound = 257 * eps * terms.to(F64).abs().sum(dim=0)
        assert bool(((got.to(F64) - ref).abs() <= bound).all()), (got, ref, bound)
    # module order (sigma, rho, beta - for these systems also the trace's compact order), y0.grad per row, t.grad
    mod = c['mod']
    assert [tuple(p.grad.shape) for p in mod.parameters()] == [(), (), ()] and all(p.grad.dtype == dtype for p in mod.parameters())
    assert torch.equal(torch.stack([mod.sigma.grad, mod.rho.grad, mod.beta.grad]), c['gp'])
    assert c['gy0'].shape == (257, 3) and c['gt'].shape == (3,) and c['gt'].dtype == F64 and bool(c['gy0'].abs().sum(dim=1).min() > 0)
    again = adjoint_call('lorenz', dtype, t=t, y0_all=y_all)
    assert torch.equal(c['gp'], again['gp']) and torch.equal(c['gt'], again['gt']) and torch.equal(c['gy0'], again['gy0'])
    one = adjoint_call('lorenz', dtype, t=t, y0_all=y_all, rows=[256])
    same_row(c, 256, one, 0)                                 # the lone lane of the second workgroup


# ---- against the existing route ------------------------------------------------------------------------------------------------------------
def test_against_odeint_adjoint_without_the_option():
    """odeint_adjoint(func, y0[i:i+1], t) without the option is the same algorithm with autograd vjps (shared control over one row IS
    per-trajectory control)."""
    t = PC.BASE_T[:3]
    c = adjoint_call('lorenz', F64, t=t)
    for i in (0, 35, 69):
        mod = AC.LorenzModule(F64, DEV)
        y0 = PC.base_y0()[i:i + 1].to(DEV).requires_grad_(True)
        tt = torch.tensor(t, dtype=F64, requires_grad=True)
        sol = odeint_adjoint(mod, y0, tt, method='dopri5', **TOL[F64])
        band64(sol.detach()[:, 0].cpu().numpy(), c['sol'][:, i].cpu().numpy(), 'row %d forward' % i)
        (torch.sin(sol) * weights(3, [i], 3, F64)).sum().backward()
        assert 'k_rows_adjoint' not in str(odeint_adjoint.last_backward_stats.get('engine'))
        band64(y0.grad[0].cpu().numpy(), c['gy0'][i].cpu().numpy(), 'row %d grad_y0' % i)
        band64(torch.stack([p.grad for p in mod.parameters()]).cpu().numpy(), c['st']['rows']['grad_params'][i].cpu().numpy(), 'row %d grad_params' % i)
        band64(tt.grad.numpy(), c['st']['rows']['time_vjps'][i].cpu().numpy(), 'row %d time_vjps' % i)


# ---- the dLd_cur_t terms ---------------------------------------------------------------------------------------------------------------------
def test_a_loss_that_reads_only_the_last_output():
    every, last = adjoint_call('lorenz', F64, rows=PC.BASE_ROWS), adjoint_call('lorenz', F64, rows=PC.BASE_ROWS, every=False)
    assert bool((last['g'][:-1] == 0).all()) and bool((every['g'][:-1] != 0).any())
    tv = last['st']['rows']['time_vjps']
    assert bool((tv[:, 1:-1] == 0).all()) and bool((tv[:, -1] != 0).all()) and bool((tv[:, 0] != 0).all())
    assert bool((every['st']['rows']['time_vjps'][:, 1:-1] != 0).all())
    for j in (0, 5):
        got, ref = row_np(last, j), oracle_row('lorenz', last, j, np.float64, TOL[F64])
        assert got[3:] == tuple(ref[3:]), (j, got[3:], ref[3:])
        for a, b, what in zip(got[:3], ref[:3], ('grad_y0', 'grad_params', 'time_vjps')):
            band64(a, b, 'last-only row %d %s' % (j, what))


# ---- a row that cannot finish ----------------------------------------------------------------------------------------------------------------
def test_a_row_that_cannot_finish_raises_the_reference_message():
    mod = AC.LorenzModule(F64, DEV)
    y0 = PC.base_y0().to(DEV).requires_grad_(True)
    sol = odeint_adjoint(mod, y0, torch.tensor(PC.BASE_T), method='dopri5', options=AC.ON, adjoint_options={'max_num_steps': 3}, **TOL[F64])
    with pytest.raises(AssertionError) as e:                 # (the kernel returns by attempt_tail's status exit: no fault, no hang)
        sol.sum().backward()
    assert 'max_num_steps exceeded (3>=3)' in str(e.value) and '70 of 70 rows failed' in str(e.value) and 'rows 0, 1, 2' in str(e.value), str(e.value)
    ok = adjoint_call('lorenz', F64, rows=[0])               # the next call is unaffected (the ticket word is the call's own)
    assert int(ok['st']['rows']['status'][0]) == 0


# ---- both methods, the time-dependent system -----------------------------------------------------------------------------------------------
def test_bosh3_against_the_oracle():
    tol, t = dict(rtol=1e-4, atol=1e-7), PC.BASE_T * 0.05
    c = adjoint_call('lorenz', F64, rows=PC.BASE_ROWS, t=t, method='bosh3', tol=tol)
    assert 'k_rows_adjoint<double, 3' in c['st']['kernel']
    for j in (1, 4):
        got, ref = row_np(c, j), oracle_row('lorenz', c, j, np.float64, tol, 'bosh3', t)
        assert got[3:] == tuple(ref[3:]), (j, got[3:], ref[3:])
        for a, b, what in zip(got[:3], ref[:3], ('grad_y0', 'grad_params', 'time_vjps')):
            band64(a, b, 'bosh3 row %d %s' % (j, what))
    f32 = adjoint_call('lorenz', F32, rows=PC.BASE_ROWS, t=t, method='bosh3', tol=tol)
    assert 'k_rows_adjoint<float, 3' in f32['st']['kernel']
    assert observed(f32['gy0'].cpu().numpy(), c['gy0'].cpu().numpy()) <= 1e-2


@pytest.mark.parametrize('n_t', [4, 2])
def test_the_time_dependent_system_against_the_oracle(n_t):
    """df/dt is not zero: the adj_t component moves and takes part in the control.  9 rows, T = 4 and T = 2."""
    t = AC.TIME_T[:n_t]
    c = adjoint_call('time', F64, t=t)
    assert c['gp'].shape == (4,) and c['gy0'].shape == (9, 3)
    mod = c['mod']
    assert torch.equal(torch.cat([mod.a.grad.reshape(1), mod.c.grad]), c['gp']) and mod.a.grad.shape == () and mod.c.grad.shape == (3,)
    for i in range(9):
        got, ref = row_np(c, i), oracle_row('time', c, i, np.float64, TOL[F64], t=t)
        assert got[3:] == tuple(ref[3:]), (i, got[3:], ref[3:])
        for a, b, what in zip(got[:3], ref[:3], ('grad_y0', 'grad_params', 'time_vjps')):
            band64(a, b, 'time row %d %s' % (i, what))
    assert bool((c['st']['rows']['time_vjps'][:, 0] != 0).all())
    one = adjoint_call('time', F64, t=t, rows=[4])
    same_row(c, 4, one, 0)
    f32 = adjoint_call('time', F32, t=t)
    assert observed(f32['gy0'].cpu().numpy(), c['gy0'].cpu().numpy()) <= 1e-2 and observed(f32['gp'].cpu().numpy(), c['gp'].cpu().numpy()) <= 1e-2
