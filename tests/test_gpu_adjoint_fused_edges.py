"""GPU tests of the fused MLP adjoint kernel (csrc/mi_ode_adjoint.h, k_adjoint_mlp<DP, HP, ACT, 6>) where tests/test_gpu_adjoint_fused.py does
not look: segments on every one of its four geometries (16 x 16, 16 x 128, 64 x 16, 64 x 128; widths at both ends and inside of each one's
range) with every activation, time dependent and not, in both time directions; grids of 1, 2 and around the unrolled slice fold's boundary up
to one workgroup per compute unit, with a second and a third tile on workgroup 0 (natural and through MI_ODE_ADJOINT_GRID); rejected
attempts - of the first attempt, after accepted steps, and one that covers t_end -; the finite-h0 branch of the initial step; a long
interval; one handle across the three activations, other weights and both directions; the non-finite status.  Inputs and oracle runs:
tests/adjmlp_cases.py; tests/test_adjmlp_cases_host.py checks on the CPU that the inputs have the properties relied on here.

The reference is the numpy oracle (oracle/ode_numpy.odeint on the restated augmented dynamics): the float32 oracle run's attempt / accept
counts, and max |got - ref| / (1 + |ref|) of adj_y, adj_t, adj_params against the float64 oracle run on the float32-rounded inputs within
4 x max(E32, bands.case_ceiling(attempts)) (adjmlp_cases.bound_of)."""
import numpy as np
import pytest
import torch

from tests import adjmlp_cases as AC
from tests import bands

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _engine(case, max_num_steps=2 ** 31 - 1):
    from tfdiffeq_amd import adjoint as ADJ
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    return ADJ._FusedAdjointEngine(AC.batch_of(case, cus()), case.dim, case.hidden, case.rtol, case.atol, f32(0.9), f32(10.0), f32(0.2), max_num_steps,
                                   dev(), case.td)


def _tt(v):
    return torch.tensor(v, dtype=torch.float32, device=dev())


def _mlp(case, x):
    from tfdiffeq_amd import rhs
    return rhs.MLP(_tt(x.W1), _tt(x.b1), _tt(x.W2), _tt(x.b2), _tt(x.W3), _tt(x.b3), activation=case.act, time_dependent=case.td)


def _segment(eng, case, x=None):
    """One segment call of a case on `eng`: ((adj_y, adj_t, adj_params) as torch tensors on the CPU, the statistics)."""
    x = AC.inputs(case, cus()) if x is None else x
    out = eng.segment(_mlp(case, x), _tt(x.y), _tt(x.a), _tt(x.adjt), _tt(x.th), case.t0, case.t1)
    return tuple(v.cpu() for v in out), eng.stats.as_dict()


def _against_the_oracle(case, got, st, tag='', grid=None):
    """Status, counts and the three outputs of one segment call against the oracle; returns the three deviations."""
    c = cus()
    ref, counts, bound = AC.oracle(case, c, 'float64'), AC.oracle(case, c, 'float32'), AC.bound_of(case, c)
    devs = [bands.observed(g.numpy().astype(np.float64), r) for g, r in zip(got, ref[:3])]
    batch = got[0].shape[0]
    print('%s%s [k_adjoint_mlp<%d, %d, %s>, dim %d, hidden %d, batch %d, G %d]: adj_y %.3e adj_t %.3e adj_params %.3e (bound %.3e); '
          'attempts %d (oracle %d), accepted %d (oracle %d)'
          % ((case.name, tag) + AC.kernel_of(case.dim, case.hidden) + (case.act, case.dim, case.hidden, batch, AC.grid_of(batch, c) if grid is None else grid,
                                                                     devs[0], devs[1], devs[2], bound, st['n_attempts'], counts.n_attempts, st['n_accepted'], counts.n_accepted)))
    assert st['n_launches'] == 1 and st['status'] == 0, st
    assert (st['n_attempts'], st['n_accepted']) == (counts.n_attempts, counts.n_accepted), (st, counts.n_attempts, counts.n_accepted)
    assert max(devs) <= bound, (devs, bound)
    return devs


def _run(case, monkeypatch=None, grid=None):
    if grid is not None:
        monkeypatch.setenv('MI_ODE_ADJOINT_GRID', str(grid))     # (read when the engine is created)
    eng = _engine(case)
    try:
        got, st = _segment(eng, case)
    finally:
        eng.close()
    _against_the_oracle(case, got, st, '' if grid is None else ' (grid override)', grid)
    return got, st


def _rel(got, ref):
    return float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


# ---- a. every instantiation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', AC.EVERY, ids=AC.ids(AC.EVERY))
def test_every_instantiation_against_the_oracle(case):
    """The segment, and one evaluation of the augmented dynamics of the same network shape (adjmlp_cases.dynamics_inputs) against the float64
    restatement."""
    xd = AC.dynamics_inputs(case, cus())
    eng = _engine(case)
    try:
        f, vy, vp = eng.dynamics(_mlp(case, xd), _tt(xd.y), _tt(xd.a), case.t0)
        got, st = _segment(eng, case)
    finally:
        eng.close()
    rf, rvy, _, rvp = AC.dynamics_reference(case, cus())
    figs = (_rel(f, rf), _rel(vy, rvy), _rel(vp, rvp))
    print('%s: dynamics f %.3e, vjp_y %.3e, vjp_params %.3e (bar %.0e)' % ((case.name,) + figs + (AC.DYNAMICS_BAR,)))
    assert max(figs) < AC.DYNAMICS_BAR, figs
    _against_the_oracle(case, got, st)


@pytest.mark.parametrize('case', AC.TINY, ids=AC.ids(AC.TINY))
def test_one_row_and_one_ragged_tile_against_the_oracle(case):
    _run(case)


# ---- b. grids by batch size -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', AC.GRIDS, ids=AC.ids(AC.GRIDS))
def test_natural_grid_against_the_oracle(case):
    _run(case)


# ---- c. grids by override -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', AC.OVERRIDE, ids=AC.ids(AC.OVERRIDE))
def test_overridden_grids_agree_with_the_oracle_and_with_each_other(case, monkeypatch):
    runs = [_run(case, monkeypatch, g) for g in AC.OVERRIDE_GRIDS]
    first, st0 = runs[0]
    bound = AC.bound_of(case, cus())
    for g, (got, st) in zip(AC.OVERRIDE_GRIDS[1:], runs[1:]):
        assert (st['n_attempts'], st['n_accepted']) == (st0['n_attempts'], st0['n_accepted'])
        for p, q in zip(got, first):                            # (the fold order depends on the grid: close, not bit-identical)
            d = bands.observed(p.numpy(), q.numpy())
            print('%s: grid %d against grid %d: %.3e (bar %.3e)' % (case.name, g, AC.OVERRIDE_GRIDS[0], d, 2 * bound))
            assert d <= 2 * bound
    # the override took effect: one workgroup folds 24 tiles' partials in another order than 24 workgroups do - were the variable ignored,
    # all four runs would be the natural grid of 24 and bit-identical
    assert not all(torch.equal(p, q) for p, q in zip(runs[-1][0], first))


# ---- d. rejected attempts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', AC.REJECTING, ids=AC.ids(AC.REJECTING))
def test_rejected_attempts_against_the_oracle(case):
    _, st = _run(case)
    assert st['n_attempts'] > st['n_accepted']


# ---- e. the finite-h0 branch of the initial step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', AC.FINITE_H0, ids=AC.ids(AC.FINITE_H0))
def test_finite_h0_segment_against_the_oracle(case):
    assert case.adjt == 0.0 and np.isfinite(AC.oracle(case, cus()).h0)
    _run(case)


# ---- f. a long interval -----------------------------------------------------------------------------------------------------------------------
def test_long_interval_against_the_oracle():
    _, st = _run(AC.LONG)
    assert st['n_accepted'] >= 40


# ---- g. one handle, many segments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cases', [AC.HANDLE, AC.HANDLE_TD], ids=['time-independent', 'time-dependent'])
def test_one_engine_across_activations_weights_and_directions(cases):
    """... and the first case once more: the reductions are in a fixed order, so its result is bit for bit the first one - unless scratch
    (act, wpart, theta) or a sequence number of an earlier call leaks into it."""
    eng = _engine(cases[0])
    try:
        first = None
        for case in cases:
            got, st = _segment(eng, case)
            _against_the_oracle(case, got, st, ' (shared handle)')
            first = got if first is None else first
        again, st = _segment(eng, cases[0])
        _against_the_oracle(cases[0], again, st, ' (shared handle, again)')
        assert all(torch.equal(p, q) for p, q in zip(again, first))
    finally:
        eng.close()


# ---- h. status ------------------------------------------------------------------------------------------------------------------------------------
def test_nan_in_the_ragged_last_tile_raises_and_the_engine_recovers():
    case = AC.STATUS
    x = AC.inputs(case, cus())
    assert AC.last_tile_rows(x.y.shape[0]) == 4
    y = x.y.copy()
    y[-2, case.dim - 1] = np.nan                                # a row of the last, ragged tile
    eng = _engine(case)
    try:
        with pytest.raises(AssertionError):
            _segment(eng, case, x._replace(y=y))
        assert eng.stats.as_dict()['status'] & 2 and not eng.stats.as_dict()['status'] & 16      # non-finite state, not a hand-off time-out
        got, st = _segment(eng, case)
        _against_the_oracle(case, got, st, ' (after the non-finite call)')
    finally:
        eng.close()
