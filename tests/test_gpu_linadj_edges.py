"""GPU tests of the one-launch linear adjoint kernel (csrc/mi_ode_linadj.h, k_linadj<T, D>) where tests/test_gpu_linadj.py and
tests/test_gpu_linear_adjoint.py do not look: every one of its eight instantiations (tile widths 16 / 32 / 64 / 128 in float64 and float32,
dims at both ends and inside of each width's range), grids of 1, 2 and around the unrolled fold's boundary up to one workgroup per compute
unit (natural and through MI_ODE_LINADJ_GRID), rejected attempts - of the first attempt and after accepted steps -, the finite-h0 branch of
the initial step (adj_t = 0 at the interval's start), an interval of 74 steps, one handle across bias / no bias / another W / both time
directions, and the non-finite status.  Inputs and oracle runs: tests/linadj_cases.py; tests/test_linadj_cases_host.py checks on the CPU that
the inputs reject, have the h0 they are marked with and give the intended grids.

The reference is the numpy oracle (oracle/ode_numpy.odeint on the restated augmented dynamics).  float64: identical attempt / accept counts,
|got - ref| <= 1e-11 max(1, max |ref|) for adj_y, adj_t, adj_params (the long case: max(1e-11, 10 x the reference's own drift of the carried
G0 | g0)), the two host scalars to 1e-12.  float32: the float32 oracle's counts, and max |got - ref| / (1 + |ref|) against the float64 oracle
run on the float32-rounded inputs within 4 x max(E32, bands.case_ceiling(attempts)) (linadj_cases.f32_bound).  End-to-end tests compare
odeint_adjoint with the callable engine (adjoint.LINEAR_ONE_LAUNCH = False) at test_gpu_linadj.py's 1e-11."""
import numpy as np
import pytest
import torch

from tests import bands
from tests import linadj_cases as LC

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _engine(case, batch=None):
    from tfdiffeq_amd import adjoint as ADJ
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    return ADJ._LinearAdjointEngine(LC.batch_of(case, cus()) if batch is None else batch, case.dim, getattr(torch, case.dtype), case.rtol, case.atol,
                                    f32(0.9), f32(10.0), f32(0.2), 2 ** 31 - 1, str(dev()))


def _segment(eng, case, x=None):
    """One segment call of a case on `eng`: ((adj_y, adj_t, adj_params) as float64 numpy, the statistics, the two host scalars)."""
    x = LC.inputs(case, cus()) if x is None else x
    tt = lambda v: None if v is None else torch.tensor(v, dtype=getattr(torch, case.dtype), device=dev())  # noqa: E731
    out = eng.segment(tt(x.W), tt(x.b), tt(x.y), tt(x.a), tt(x.adjt), tt(x.th), case.t0, case.t1, grad_out=tt(x.g))
    return tuple(v.cpu().numpy().astype(np.float64) for v in out), eng.stats.as_dict(), eng.scalars


def _against_the_oracle(case, got, st, scalars, tag='', grid=None):
    """Counts, the three outputs and the two scalars of one segment call against the oracle; returns the worst deviation in units of the
    case's own measure."""
    c = cus()
    ref = LC.oracle(case, c, 'float64')
    counts = LC.oracle(case, c, case.dtype)
    bound = LC.bound_of(case, c)
    if case.dtype == 'float64':
        devs = [float(np.abs(g - r).max()) / max(1.0, float(np.abs(r).max())) for g, r in zip(got, ref[:3])]
        sc = [abs(scalars[0] - ref.dldt) / max(1.0, abs(ref.dldt)), abs(scalars[1] - float(ref.adj_t)) / max(1.0, abs(float(ref.adj_t)))]
        sc_bound = 1e-12
    else:
        devs = [bands.observed(g, r) for g, r in zip(got, ref[:3])]
        sc = [bands.observed(scalars[0], ref.dldt), bands.observed(scalars[1], float(ref.adj_t))]
        sc_bound = bound
    print('%s%s [k_linadj<%s, %d>, dim %d, batch %d, G %d]: adj_y %.3e adj_t %.3e adj_params %.3e (bound %.3e), scalars %.3e %.3e (bound %.0e); '
          'attempts %d (oracle %d), accepted %d (oracle %d), rejected %d'
          % (case.name, tag, case.dtype, LC.tile_width(case.dim), case.dim, got[0].shape[0], LC.grid_of(got[0].shape[0], c) if grid is None else grid, devs[0], devs[1], devs[2],
             bound, sc[0], sc[1], sc_bound, st['n_attempts'], counts.n_attempts, st['n_accepted'], counts.n_accepted, st['n_rejected']))
    assert st['n_launches'] == 1 and st['status'] == 0, st
    assert (st['n_attempts'], st['n_accepted']) == (counts.n_attempts, counts.n_accepted), (st, counts.n_attempts, counts.n_accepted)
    assert st['n_rejected'] == counts.n_attempts - counts.n_accepted
    assert max(devs) <= bound, (devs, bound)
    assert max(sc) <= sc_bound, (sc, sc_bound)
    return max(devs)


def _run(case, monkeypatch=None, grid=None):
    if grid is not None:
        monkeypatch.setenv('MI_ODE_LINADJ_GRID', str(grid))      # (read when the engine is created)
    eng = _engine(case)
    try:
        got, st, sc = _segment(eng, case)
    finally:
        eng.close()
    _against_the_oracle(case, got, st, sc, '' if grid is None else ' (grid override)', grid)
    return got, st


# ---- a. every instantiation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.EVERY + LC.TINY, ids=LC.ids(LC.EVERY + LC.TINY))
def test_every_instantiation_against_the_oracle(case):
    _run(case)


# ---- b. grids by batch size -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.GRIDS, ids=LC.ids(LC.GRIDS))
def test_natural_grid_against_the_oracle(case):
    _run(case)


# ---- c. grids by override -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.OVERRIDE, ids=LC.ids(LC.OVERRIDE))
def test_overridden_grids_agree_with_the_oracle_and_with_each_other(case, monkeypatch):
    runs = [_run(case, monkeypatch, g) for g in LC.OVERRIDE_GRIDS]
    first, st0 = runs[0]
    for g, (got, st) in zip(LC.OVERRIDE_GRIDS[1:], runs[1:]):
        assert (st['n_attempts'], st['n_accepted']) == (st0['n_attempts'], st0['n_accepted'])
        for p, q in zip(got, first):                            # (the fold order depends on G: close, not bit-identical)
            rel = float(np.abs(p - q).max()) / max(float(np.abs(q).max()), 1e-300)
            print('%s: grid %d against grid %d: %.3e' % (case.name, g, LC.OVERRIDE_GRIDS[0], rel))
            assert rel <= 1e-12


# ---- d. rejected attempts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.REJECTING, ids=LC.ids(LC.REJECTING))
def test_rejected_attempts_against_the_oracle(case):
    _, st = _run(case)
    assert st['n_rejected'] >= 1


# ---- e. the finite-h0 branch of the initial step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.FINITE_H0, ids=LC.ids(LC.FINITE_H0))
def test_finite_h0_segment_against_the_oracle(case):
    assert case.adjt == 0.0 and not case.grad and np.isfinite(LC.oracle(case, cus()).h0)
    _run(case)


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _grads(func, y0, t, w, one_launch, **kw):
    from tfdiffeq_amd import adjoint as ADJ
    from tfdiffeq_amd import odeint_adjoint
    ADJ.LINEAR_ONE_LAUNCH = one_launch
    try:
        for p in func.parameters():
            p.grad = None
        yi = y0.clone().requires_grad_(True)
        tt = t.clone().requires_grad_(True)
        sol = odeint_adjoint(func, yi, tt, **kw)
        (sol * w).sum().backward()
        return sol.detach(), yi.grad.clone(), [p.grad.clone() for p in func.parameters()], tt.grad.clone(), dict(odeint_adjoint.last_backward_stats)
    finally:
        ADJ.LINEAR_ONE_LAUNCH = True


TOL64 = dict(rtol=1e-7, atol=1e-9, method='dopri5')


def _same_gradients(a, b, name):
    assert a[4]['engine'].startswith('linear right-hand side: one launch per interval')
    assert b[4]['engine'].startswith('linear right-hand side: augmented dynamics on the MFMA kernels')
    assert all(s_['n_launches'] == 1 and s_['status'] == 0 for s_ in a[4]['segments'])
    assert a[4]['segments'][-1]['n_attempts'] == b[4]['last_segment']['n_attempts']
    figs = [_rel(a[1], b[1])] + [_rel(x, y) for x, y in zip(a[2], b[2])] + [float((a[3] - b[3]).abs().max()) / max(1.0, float(b[3].abs().max()))]
    print('%s: one launch against the callable engine: dL/dy0 %.3e, parameters %s, dL/dt %.3e (bar 1e-11)'
          % (name, figs[0], ' '.join('%.3e' % f for f in figs[1:-1]), figs[-1]))
    assert len(a[2]) == len(b[2]) and max(figs) < 1e-11, figs


def _model(dim, bias, seed):
    from tfdiffeq_amd import models
    torch.manual_seed(seed)
    func = models.LinearODEFunc(dim, bias=bias, dtype=torch.float64).to(dev())
    if bias:
        with torch.no_grad():
            func.bias.normal_(0.0, 0.1)
    return func


def _problem(batch, dim, tpts, only=None):
    g = torch.Generator().manual_seed(batch + dim)
    y0 = torch.randn(batch, dim, generator=g, dtype=torch.float64).to(dev())
    w = torch.randn(len(tpts), batch, dim, generator=g, dtype=torch.float64)
    if only is not None:
        keep = torch.zeros_like(w)
        keep[only] = w[only]
        w = keep
    return y0, torch.tensor(tpts, dtype=torch.float64), w.to(dev())


@pytest.mark.parametrize('dim,bias', [(20, True), (100, False)])
def test_loss_on_a_middle_output_starts_the_newest_interval_from_zero(dim, bias):
    """Only y(0.6) is weighted: the interval 1.0 -> 0.6 starts from adj_y = 0, adj_t = 0, adj_params = 0 - a finite h0 - and is the y system
    alone; its attempt count is the oracle's on that state, the last interval's the callable engine's."""
    from tfdiffeq_amd import adjoint as ADJ
    ADJ.clear_adjoint_engines()
    try:
        batch = 200
        func = _model(dim, bias, dim)
        y0, t, w = _problem(batch, dim, [0.0, 0.6, 1.0], only=1)
        a = _grads(func, y0, t, w, True, **TOL64)
        b = _grads(func, y0, t, w, False, **TOL64)
        _same_gradients(a, b, 'middle output, dim %d' % dim)
        segs = a[4]['segments']
        assert len(segs) == 2
        W = func.weight.detach().cpu().numpy()
        bb = func.bias.detach().cpu().numpy() if bias else None
        zeros = np.zeros((batch, dim))
        x = LC.Inputs(W, bb, a[0][2].cpu().numpy(), zeros, None, np.array(0.0), np.zeros(dim * dim + (dim if bias else 0)))
        ref = LC.run_oracle(x, 1.0, 0.6, TOL64['rtol'], TOL64['atol'])
        assert np.isfinite(ref.h0)
        print('middle output, dim %d: newest interval %d attempts / %d accepted (oracle %d / %d, h0 %.3g)'
              % (dim, segs[0]['n_attempts'], segs[0]['n_accepted'], ref.n_attempts, ref.n_accepted, ref.h0))
        assert (segs[0]['n_attempts'], segs[0]['n_accepted']) == (ref.n_attempts, ref.n_accepted)
    finally:
        ADJ.clear_adjoint_engines()


# ---- f. a long interval -----------------------------------------------------------------------------------------------------------------------
def test_long_interval_against_the_oracle():
    _, st = _run(LC.LONG)
    assert st['n_accepted'] >= 60


# ---- g. one handle, many segments ---------------------------------------------------------------------------------------------------------
def test_one_engine_across_bias_no_bias_another_matrix_and_both_directions():
    eng = _engine(LC.HANDLE[0])
    try:
        for case in LC.HANDLE:
            got, st, sc = _segment(eng, case)
            _against_the_oracle(case, got, st, sc, ' (shared handle)')
    finally:
        eng.close()


def test_two_models_share_one_cached_engine():
    from tfdiffeq_amd import adjoint as ADJ
    ADJ.clear_adjoint_engines()
    try:
        y0, t, w = _problem(250, 20, [0.0, 0.4, 1.0])
        with_b, without_b = _model(20, True, 5), _model(20, False, 6)
        one = [_grads(f, y0, t, w, True, **TOL64) for f in (with_b, without_b, with_b)]
        assert len(ADJ._LIN_ENGINES) == 1                       # (the cache key has no bias in it: one handle served all three)
        ref = [_grads(f, y0, t, w, False, **TOL64) for f in (with_b, without_b)]
        _same_gradients(one[0], ref[0], 'shared engine, bias')
        _same_gradients(one[1], ref[1], 'shared engine, no bias after bias')
        _same_gradients(one[2], ref[0], 'shared engine, bias after no bias')
    finally:
        ADJ.clear_adjoint_engines()


def test_weight_updated_in_place_between_two_backward_passes():
    from tfdiffeq_amd import adjoint as ADJ
    ADJ.clear_adjoint_engines()
    try:
        y0, t, w = _problem(250, 33, [0.0, 0.5, 1.0])
        func = _model(33, True, 7)
        before = _grads(func, y0, t, w, True, **TOL64)
        with torch.no_grad():
            func.weight.mul_(1.5)
        after = _grads(func, y0, t, w, True, **TOL64)
        assert len(ADJ._LIN_ENGINES) == 1
        ref = _grads(func, y0, t, w, False, **TOL64)
        _same_gradients(after, ref, 'weight.mul_(1.5)')
        assert _rel(after[2][0], before[2][0]) > 1e-3           # (the update changed the gradient: the second pass did not reuse the first's matrices)
    finally:
        ADJ.clear_adjoint_engines()


# ---- h. status ------------------------------------------------------------------------------------------------------------------------------------
def test_nan_in_the_ragged_last_tile_raises_and_the_engine_recovers():
    case = LC.STATUS
    x = LC.inputs(case, cus())
    assert LC.last_tile_rows(x.y.shape[0]) == 4
    y = x.y.copy()
    y[-2, case.dim - 1] = np.nan                                # a row of the last, ragged tile
    eng = _engine(case)
    try:
        with pytest.raises(AssertionError):
            _segment(eng, case, x._replace(y=y))
        assert eng.stats.as_dict()['status'] & 2 and not eng.stats.as_dict()['status'] & 16      # non-finite state, not a hand-off time-out
        got, st, sc = _segment(eng, case)
        _against_the_oracle(case, got, st, sc, ' (after the non-finite call)')
    finally:
        eng.close()
