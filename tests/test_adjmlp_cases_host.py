"""CPU checks of the inputs of tests/test_gpu_adjoint_fused_edges.py (tests/adjmlp_cases.py), from the oracle alone: the numpy restatement of
the augmented dynamics is torch.autograd's (float64, 1e-12) for every activation, time dependent and not; every case passes the admission
conditions (a) - (g) of adjmlp_cases.admission - the float32 and the float64 oracle run take the same decisions, farther than 0.02 from the
threshold and farther than they disagree about a ratio, with step sizes within 5 % of each other, no step boundary near t_end, outputs of
moderate size and a bound below 1e-3 -; one evaluation's inputs leave a plain float32 evaluation within a quarter of the 3e-6 bar; the
rejecting cases reject after an accepted step on all four kernels, one its first attempt, one with a rejected attempt across t_end; the first
guess h0 is finite exactly where adj_t = 0 or the network is time dependent; the long case is long; every kernel sees every activation, both
time-dependence settings and both directions; every batch gives the grid and the last-tile row count it is there for - so that a GPU
failure cannot be blamed on the inputs."""
import math

import numpy as np
import pytest
import torch

from tests import adjmlp_cases as AC

CUS = AC.DEFAULT_CUS


@pytest.mark.parametrize('td', [False, True], ids=['ti', 'td'])
@pytest.mark.parametrize('act', ['tanh', 'relu', 'softplus'])
def test_restatement_is_autograd(act, td):
    from tfdiffeq_amd.models import ODEFunc
    case = AC._mk('autograd', 7, 11, 37, (0.7, 0.0), act=act, td=td, seed=3, yscale=12.0 if act == 'softplus' else 4.0)
    x = AC.inputs(case, dtype='float64')
    func = ODEFunc(case.dim, case.hidden, non_linearity=act, time_dependent=td).double()
    with torch.no_grad():
        for lin, W, b in ((func.fc1, x.W1, x.b1), (func.fc2, x.W2, x.b2), (func.fc3, x.W3, x.b3)):
            lin.weight.copy_(torch.tensor(W).t())
            lin.bias.copy_(torch.tensor(b))
    t = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    y = torch.tensor(x.y, requires_grad=True)
    f = func(t, y)
    if act == 'softplus':                                   # (both sides of the threshold are exercised)
        z1 = x.y @ x.W1[1 if td else 0:] + x.b1 + (0.7 * x.W1[0] if td else 0.0)
        assert (z1 > 20).any() and (z1 < 20).any()
    grads = torch.autograd.grad(f, (t, y) + tuple(func.parameters()), torch.tensor(-x.a), allow_unused=True)
    w1, b1, w2, b2, w3, b3 = (g.numpy() for g in grads[2:])
    canon = np.concatenate([w1.T.reshape(-1), b1, w2.T.reshape(-1), b2, w3.T.reshape(-1), b3])      # ([1 + dim, hidden]: row 0 = w_t first)
    rf, rvy, rvt, rvp = AC.augmented(x, act, td)(np.float64(0.7), (x.y, x.a, x.adjt, x.th))
    assert rvp.shape == (AC.n_params(case.dim, case.hidden, td),)
    for got, ref in ((rf, f.detach().numpy()), (rvy, grads[1].numpy()), (rvp, canon), (rvt, grads[0].numpy() if td else np.zeros(()))):
        assert got.shape == ref.shape
        assert float(np.abs(got - ref).max()) <= 1e-12 * max(1.0, float(np.abs(ref).max()))
    assert (grads[0] is None) == (not td) and (not td or float(abs(rvt)) > 0.0)


def test_dynamics_inputs_suit_the_bar():
    """One evaluation is held to 3e-6 of the float64 restatement: on its inputs a plain float32 evaluation stays within a quarter of that."""
    worst = {c.name: AC.dynamics_f32_error(c) for c in AC.EVERY}
    print('float32 restatement against float64, one evaluation: worst %.3e (%s)' % (max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= AC.DYNAMICS_BAR / 4, worst
    for c in AC.EVERY[:3]:
        xd, x = AC.dynamics_inputs(c), AC.inputs(c)
        assert xd.y.shape == x.y.shape and xd.W1.shape == x.W1.shape and 0.5 < float(np.abs(xd.a).max()) < 6.0


@pytest.mark.parametrize('case', AC.SEGMENT_CASES, ids=AC.ids(AC.SEGMENT_CASES))
def test_case_is_admitted(case):
    fig, fails = AC.admission(case)                         # (an oracle assertion - dt underflow, non-finite state - fails the test here)
    lo, hi = AC.oracle(case, dtype='float32'), AC.oracle(case, dtype='float64')
    print('%s: %s, %d attempts, %d accepted, h0 %g; ratio gap %.3f (the runs disagree by %.3f), dt_next agreement %.1e, end gap %.1e, max |adj_params| %.1e; E32 %.3e, '
          'ceiling %.3e, bound %.3e' % (case.name, fig['seq32'], lo.n_attempts, lo.n_accepted, lo.h0, fig['gap'], fig['noise'], fig.get('dt_next', math.nan),
                                        fig['end_gap'], fig['max_theta'], fig['e32'], AC.bands.case_ceiling(lo.n_attempts), fig['bound']))
    assert not fails, (fails, fig)
    batch = AC.batch_of(case)
    assert hi.adj_y.shape == (batch, case.dim) and hi.adj_params.shape == (AC.n_params(case.dim, case.hidden, case.td),) and hi.adj_t.shape == ()
    assert len(lo.ratios) == lo.n_attempts >= 2 and all(len(r) == 4 for r in lo.ratios)
    assert [max(r) <= 1.0 for r in lo.ratios] == [bool(row[2]) for row in lo.trace]
    assert fig['bound'] == 4.0 * max(fig['e32'], AC.bands.case_ceiling(lo.n_attempts))
    # the first guess h0 of the initial step: finite where adj_t = 0 - and in every time-dependent case, where adj_t has a derivative
    assert case.finite_h0 == (case.adjt == 0.0)
    for r in (lo, hi):
        assert math.isfinite(r.h0) == (case.finite_h0 or case.td), r.h0
        assert r.h0 > 0.0
    if case.td:
        assert float(hi.adj_t) != case.adjt                 # (it evolves)
    if case.rejecting:
        assert 'Ar' in fig['seq32'], fig['seq32']           # a rejection AFTER an accepted step


def test_no_two_cases_are_the_same_input():
    keys = [c._replace(name='', rejecting=False, finite_h0=False) for c in AC.SEGMENT_CASES]
    assert len(set(keys)) == len(keys)


def test_rejecting_cases_cover_every_kernel_a_first_attempt_and_a_covered_t_end():
    assert {AC.kernel_of(c.dim, c.hidden) for c in AC.REJECTING[:4]} == set(AC.BOXES)
    assert all(c.batch == 100 for c in AC.REJECTING[:4]) and any(c.batch == 'FULL' for c in AC.REJECTING)
    for dt in ('float32', 'float64'):
        assert AC.accepts(AC.oracle(AC.REJECT_FIRST, dtype=dt)).startswith('r')
    # the covered t_end: the case is the (8, 32) rejecting case up to the rejected attempt 9, whose span holds t_end
    base, cov = AC.ALL_CASES['rej-d8-h32-tanh-ti-down'], AC.COVERED_T_END
    assert cov._replace(name=base.name, t1=base.t1) == base
    for dt in ('float32', 'float64'):
        rb, rc = AC.oracle(base, dtype=dt), AC.oracle(cov, dtype=dt)
        assert rc.trace[:9] == rb.trace[:9] and rc.trace[9][:3] == rb.trace[9][:3]
        t0_r, dt_r, accepted = rc.trace[9][:3]
        t_end = -cov.t1
        assert not accepted and any(row[2] for row in rc.trace[:9])
        assert t0_r < t_end < t0_r + dt_r
        assert 0.89 < (t_end - t0_r) / dt_r < 0.91          # (t_end = t0_r + 0.9 dt_r of the float32 run)
        assert rc.n_attempts > 10


def test_finite_h0_cases_cover_zero_and_small_theta_time_dependent_and_not():
    assert sorted((c.th0 == 0.0, c.td) for c in AC.FINITE_H0) == [(False, False), (False, True), (True, False), (True, True)]
    assert all(c.adjt == 0.0 and c.finite_h0 for c in AC.FINITE_H0)
    assert not any(c.finite_h0 for c in AC.SEGMENT_CASES if c not in AC.FINITE_H0)
    for c in AC.FINITE_H0:                                  # the d1 <= 1e-15 corner is not here (tests/test_gpu_adjoint_fused.py has it)
        x = AC.inputs(c, dtype='float64')
        assert float(np.abs(x.a).max()) > 0.0


def test_long_case_is_long():
    c = AC.LONG
    assert (c.dim, c.hidden, c.act) == (8, 32, 'tanh')
    for dt in ('float32', 'float64'):
        assert AC.oracle(c, dtype=dt).n_accepted >= 40


def test_every_kernel_has_its_widths_activations_time_dependence_and_directions():
    assert len(AC.EVERY) == 28
    for kernel, dims in AC.BOXES.items():
        box = [c for c in AC.EVERY if (c.dim, c.hidden) in dims]
        assert len(box) == 7 and {(c.dim, c.hidden) for c in box} == set(dims)
        assert all(AC.kernel_of(c.dim, c.hidden) == kernel for c in box)
        assert {c.act for c in box} == {'tanh', 'relu', 'softplus'} and {c.td for c in box} == {True, False}
        assert any(c.t1 < c.t0 for c in box) and any(c.t1 > c.t0 for c in box)
    assert sorted(AC.BOXES) == [(16, 16), (16, 128), (64, 16), (64, 128)]
    # the selection edges: dim 16 | 17, hidden 16 | 17, dim 1, hidden 1, dim 64 and hidden 128 alone
    have = {(c.dim, c.hidden) for c in AC.EVERY}
    assert {(1, 1), (16, 16), (16, 17), (17, 16), (17, 17), (1, 17), (17, 1), (64, 16), (9, 128), (64, 128)} <= have
    assert all(c.batch == 100 for c in AC.EVERY) and AC.n_tiles(100) == 4 and AC.last_tile_rows(100) == 4
    assert sorted((c.dim, c.hidden, c.batch) for c in AC.TINY) == [(3, 5, 1), (3, 5, 31), (64, 128, 1), (64, 128, 31)]
    assert (AC.block_of(16, 16), AC.block_of(9, 128), AC.block_of(64, 16), AC.block_of(64, 128)) == (128, 512, 512, 512)


@pytest.mark.parametrize('cus', [256, 304, 64])
def test_batches_give_the_intended_grids_and_last_tiles(cus):
    want = {}
    for c in AC.GRIDS:
        b = c.batch
        want[c.name] = b[1] if isinstance(b, tuple) else cus - 1 if b == 'CUS-1' else cus
    assert sorted(want[c.name] for c in AC.GRIDS if c.dim == 12) == list(AC.GRIDS_16)
    assert sorted(want[c.name] for c in AC.GRIDS if c.dim == 40) == list(AC.GRIDS_64)
    # the 8-way unrolled fold of adj_slice: thread group q of blockDim / 128 takes workgroups q, q + groups, ... - 8 at a time while
    # q + 7 groups < G; the grids sit on both sides of G = 8 groups, and of G = 7 groups + 1 where only group 0 unrolls
    for dims, grids in (((12, 14), AC.GRIDS_16), ((40, 100), AC.GRIDS_64)):
        groups = AC.block_of(*dims) // 128
        assert {7 * groups, 7 * groups + 1, 8 * groups, 8 * groups + 1} <= set(grids) and 1 in grids and max(grids) > 15 * groups
    for c in AC.GRIDS:
        b = AC.batch_of(c, cus)
        if want[c.name] <= cus:                             # (a device with fewer compute units than a fixed G caps that grid: still a legal case)
            assert AC.grid_of(b, cus) == want[c.name], c.name
        if c.batch not in ('FULL', 'FULL3'):
            assert AC.n_tiles(b) == want[c.name] and AC.last_tile_rows(b) == 11, c.name
    full, full3 = AC.batch_of('FULL', cus), AC.batch_of('FULL3', cus)
    assert AC.n_tiles(full) == cus + 1 and AC.last_tile_rows(full) == 11 and AC.grid_of(full, cus) == cus
    assert AC.n_tiles(full3) == 2 * cus + 1 and AC.last_tile_rows(full3) == 1 and AC.grid_of(full3, cus) == cus
    assert sorted((c.dim, c.hidden) for c in AC.SEGMENT_CASES if c.batch == 'FULL') == [(16, 16), (16, 16), (64, 128)]
    assert [(c.dim, c.hidden) for c in AC.SEGMENT_CASES if c.batch == 'FULL3'] == [(16, 16)]
    # (3, 5): 68 parameters, a slice of one per workgroup on a full grid - the workgroups from 68 on own no theta
    p35 = AC.n_params(3, 5, False)
    assert p35 == 68 and all((c.dim, c.hidden, c.td) == (3, 5, False) for c in AC.GRIDS if c.batch in ('CUS', 'CUS-1') and c.dim == 3)
    if cus - 1 > p35:
        assert -(-p35 // (cus - 1)) == 1
    for c in AC.OVERRIDE:
        assert c.batch == 745 and AC.n_tiles(745) == 24 and AC.last_tile_rows(745) == 9 and max(AC.OVERRIDE_GRIDS) == 24 <= cus
        assert AC.n_params(c.dim, c.hidden, c.td) > 8 * 128      # grid 1: the slice is all of theta, many 128-element chunks
    assert 24 % 5 != 0 and AC.OVERRIDE_GRIDS == (1, 2, 5, 24)    # grid 5: unequal tile counts
    assert [(c.dim, c.hidden) for c in AC.OVERRIDE] == [(10, 24), (48, 96)]


def test_handle_cases_share_one_engine_key():
    for cases, td in ((AC.HANDLE, False), (AC.HANDLE_TD, True)):
        assert len({(c.batch, c.dim, c.hidden, c.rtol, c.atol, c.td) for c in cases}) == 1 and cases[0].td == td
        assert [c.act for c in cases] == ['tanh', 'relu', 'softplus', 'tanh', 'tanh', 'tanh']
        assert not np.array_equal(AC.inputs(cases[0]).W2, AC.inputs(cases[3]).W2)
        assert cases[4].t1 > cases[4].t0 and cases[5].t1 < cases[5].t0
    assert AC.last_tile_rows(AC.STATUS.batch) == 4
