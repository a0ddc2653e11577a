"""CPU checks of the inputs of tests/test_gpu_linadj_edges.py (tests/linadj_cases.py), from the oracle alone: the rejecting cases reject (one
of them at least twice, one per tile width of k_linadj<T, D>), the finite-h0 cases - and only they - have a finite first guess h0 in the
initial step, the long case has 60 accepted steps, the float32 cases take the same attempts in the float32 and the float64 oracle run, every
attempt's error ratio is decided (farther than 1e-9 from 1: a summation-order difference on the device cannot fork the accept / reject
sequence), every bound is finite, and every batch gives the grid and the last-tile row count it is there for - so that a GPU failure cannot
be blamed on the inputs."""
import math

import numpy as np
import pytest

from tests import linadj_cases as LC

CUS = LC.DEFAULT_CUS


@pytest.mark.parametrize('case', LC.SEGMENT_CASES, ids=LC.ids(LC.SEGMENT_CASES))
def test_case_is_clean_decided_and_bounded(case):
    r = LC.oracle(case)                                     # (an oracle assertion - dt underflow, non-finite state - fails the test here)
    batch = LC.batch_of(case)
    assert r.adj_y.shape == (batch, case.dim) and r.adj_params.shape == (case.dim * case.dim + (case.dim if case.bias else 0),)
    assert all(np.isfinite(v).all() for v in r[:3])
    assert len(r.ratios) == r.n_attempts >= 2
    assert [q <= 1.0 for q in r.ratios] == [bool(row[2]) for row in r.trace]
    gap = float(np.min(np.abs(np.array(r.ratios) - 1.0)))
    assert gap > (1e-9 if case.dtype == 'float64' else 1e-3), (gap, r.ratios)
    # 1e-11 relative to max |ref| is a float64 statement only while the outputs stay of moderate size
    assert float(np.abs(r.adj_params).max()) <= 1e3 and float(np.abs(r.adj_y).max()) <= 2e3
    if case.rejecting:
        assert r.n_attempts > r.n_accepted, r.ratios
    if case.finite_h0:
        assert math.isfinite(r.h0) and r.h0 > 0.0
    else:
        assert r.h0 == math.inf
    bound = LC.bound_of(case)
    print('%s: %d attempts, %d accepted, h0 %g, bound %.3e' % (case.name, r.n_attempts, r.n_accepted, r.h0, bound))
    assert math.isfinite(bound) and 0.0 < bound < 1e-3


F32 = [c for c in LC.SEGMENT_CASES if c.dtype == 'float32']


@pytest.mark.parametrize('case', F32, ids=LC.ids(F32))
def test_float32_case_takes_the_same_attempts_in_both_precisions(case):
    lo, hi = LC.oracle(case, dtype='float32'), LC.oracle(case, dtype='float64')
    assert (lo.n_attempts, lo.n_accepted) == (hi.n_attempts, hi.n_accepted)
    assert [row[2] for row in lo.trace] == [row[2] for row in hi.trace]
    assert float(np.min(np.abs(np.array(lo.ratios) - 1.0))) > 1e-3, lo.ratios          # decided in float32 too
    assert lo.h0 == hi.h0 == math.inf
    e32, bound = LC.f32_error(case), LC.f32_bound(case)
    print('%s: E32 %.3e, a-priori ceiling %.3e, bound %.3e' % (case.name, e32, LC.bands.case_ceiling(lo.n_attempts), bound))
    assert bound == 4.0 * max(e32, LC.bands.case_ceiling(lo.n_attempts)) and math.isfinite(bound)


def test_rejecting_cases_cover_every_tile_width_and_reject_twice_somewhere():
    assert {LC.tile_width(c.dim) for c in LC.REJECTING if c.dtype == 'float64'} == {16, 32, 64, 128}
    assert [c.dim for c in LC.REJECTING if c.dtype == 'float64' and c.batch != 'FULL'] == [12, 24, 40, 100]
    assert any(c.dtype == 'float32' for c in LC.REJECTING) and any(c.batch == 'FULL' for c in LC.REJECTING)
    rejected = {c.name: LC.oracle(c).n_attempts - LC.oracle(c).n_accepted for c in LC.REJECTING}
    assert max(rejected.values()) >= 2, rejected
    # a rejection AFTER an accepted step (the planes, G0 and adj_params of a later start state must stay put), not only of the first attempt
    for c in LC.REJECTING:
        if c.dtype == 'float64':
            acc = [bool(row[2]) for row in LC.oracle(c).trace]
            assert any(acc[i - 1] and not acc[i] for i in range(1, len(acc))), (c.name, acc)


def test_long_case_is_long_and_its_bound_comes_from_the_reference():
    r = LC.oracle(LC.LONG)
    assert r.n_accepted >= 60
    drift, bound = LC.carried_g0_drift(LC.LONG), LC.long_bound(LC.LONG)
    print('long case: %d accepted steps, carried G0 | g0 against the states\' own products: relative drift %.3e, bound %.3e' % (r.n_accepted, drift, bound))
    assert math.isfinite(drift) and bound == max(1e-11, 10.0 * drift) and bound < 1e-9


def test_every_instantiation_has_its_dims_and_both_directions():
    for dt in ('float64', 'float32'):
        fam = [c for c in LC.EVERY if c.dtype == dt]
        assert sorted({c.dim for c in fam}) == [1, 3, 16, 17, 20, 32, 33, 48, 64, 65, 127, 128]
        for width, dims in LC.BOXES.items():
            box = [c for c in fam if c.dim in dims]
            assert all(LC.tile_width(c.dim) == width for c in box) and len(box) == 6
            assert {c.bias for c in box} == {True, False}
            assert any(c.t1 < c.t0 for c in box) and any(c.t1 > c.t0 for c in box)
        assert all(c.grad and c.batch == 100 for c in fam)
    assert LC.n_tiles(100) == 7 and LC.last_tile_rows(100) == 4
    assert sorted((c.dtype, c.dim, c.batch) for c in LC.TINY) == sorted((dt, d, b) for dt in ('float64', 'float32') for d in (3, 128) for b in (1, 15))


@pytest.mark.parametrize('cus', [256, 304, 64])
def test_batches_give_the_intended_grids_and_last_tiles(cus):
    want = {'grid-d20-G%d' % g: g for g in (1, 2, 7, 8, 49, 50, 56, 57, 105)}
    want.update({'grid-d20-GCUS-1': cus - 1, 'grid-d20-GCUS': cus, 'grid-d128-G1': 1, 'grid-d128-G2': 2, 'grid-d128-G50': 50, 'grid-d128-GCUS': cus,
                 'grid-d5-GCUS': cus, 'grid-d16-GCUS': cus, 'grid-32-d20-GCUS': cus})
    assert sorted(want) == sorted(c.name for c in LC.GRIDS)
    for c in LC.GRIDS:
        b = LC.batch_of(c, cus)
        if want[c.name] <= cus:                             # (a device with fewer compute units than a fixed G caps that grid: still a legal case)
            assert LC.grid_of(b, cus) == min(want[c.name], LC.MAX_G), c.name
        assert LC.last_tile_rows(b) == 11, c.name
    full = LC.batch_of('FULL', cus)
    assert LC.n_tiles(full) == cus + 1 and LC.last_tile_rows(full) == 11 and LC.grid_of(full, cus) == min(cus, LC.MAX_G)
    for c in LC.OVERRIDE:
        assert c.batch == 369 and LC.n_tiles(369) == 24 and LC.last_tile_rows(369) == 1 and max(LC.OVERRIDE_GRIDS) == 24
    # a full grid at dim <= 16: E = 272 entries of adj_params in the padded layout, ceil(E / G) each - the last workgroups own none
    if cus >= 137:
        epw = -(-272 // min(cus, LC.MAX_G))
        assert epw * (min(cus, LC.MAX_G) - 1) >= 272


def test_handle_cases_share_one_engine_key():
    assert len({(c.batch, c.dim, c.dtype, c.rtol, c.atol) for c in LC.HANDLE}) == 1
    assert [c.bias for c in LC.HANDLE[:3]] == [True, False, True] and LC.HANDLE[3].t1 < LC.HANDLE[3].t0 and LC.HANDLE[4].t1 > LC.HANDLE[4].t0
    assert not np.array_equal(LC.inputs(LC.HANDLE[0]).W, LC.inputs(LC.HANDLE[2]).W)
    assert LC.last_tile_rows(LC.STATUS.batch) == 4


def test_adj_params_decides_the_first_step_of_the_theta_cases():
    """The finite-h0 branch forms adj_params' second evaluation from four of the M_pq: in these cases that number decides the first step size,
    so a wrong combination changes the whole solution; the oracle's first attempt takes exactly that step."""
    cases = [c for c in LC.FINITE_H0 if c.name.startswith('h0-theta')]
    assert {LC.tile_width(c.dim) for c in cases} == {32, 128} and {c.t1 > c.t0 for c in cases} == {True, False}
    for c in cases:
        full, without = LC.theta_decides_first_step(c)
        print('%s: first step %.6g, without the adj_params component %.6g' % (c.name, full, without))
        assert full < 0.9 * without
        assert LC.oracle(c).trace[0][1] == full
