"""CPU checks of the inputs of tests/test_gpu_conv_edges.py (tests/conv_cases.py), from the restatement and the oracle alone: the float32
restatement and the three planted defects are what they claim to be; the evaluation cases cover every F, C, image and batch class in each
of the twelve kernel instantiations; every case has an output of O(1) and tells each planted defect from float32 rounding by a factor of
ten over its own float32 bound; the saturation cases saturate; the solve cases are decided by truncation error, not roundoff (same accept /
reject sequence in float32 and float64, no error ratio within 0.02 of 1, no step boundary within 1e-3 of an output time) and the rejecting
ones reject where they are meant to; and mi_ode_conv_stage refuses every malformed descriptor before it launches anything - so that a GPU
failure cannot be blamed on the inputs."""
import ctypes as C

import numpy as np
import pytest

from tests import bands
from tests import conv_cases as CC
from tests import conv_restatement as CR
from tfdiffeq_amd import _native as N


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', CC.ACTS)
@pytest.mark.parametrize('td', [False, True], ids=['ti', 'td'])
def test_f32_restatement_is_float32_and_close(act, td):
    c = CC.Eval('float32', act, td, 2, 3, 7, 6, 17)
    p, y = list(CC.params(c)), CC.state(c)
    lo, hi = CR.f32(p, 0.7, y, act, td), CR.f(p, 0.7, y, act, td)
    assert lo.dtype == np.float32 and hi.dtype == np.float64 and lo.shape == hi.shape == y.shape
    d = bands.observed(lo, hi)
    assert 0.0 < d <= 2e-6, d                            # float32 all the way (not a rounded float64 result), and no worse than a few ulps


@pytest.mark.parametrize('act', CC.ACTS)
def test_planted_defects_change_what_they_name_and_nothing_else(act):
    c = CC.Eval('float64', act, True, 2, 3, 6, 7, 17)
    p, y = list(CC.params(c)), CC.state(c)
    good = CR.f(p, 0.7, y, act, True)
    assert np.array_equal(good, CR.f(p, 0.7, y, act, True, defect=None))
    for d in ('time_taps_unclipped', 'halo_is_act_b1'):   # border code: the interior pixels are bit-identical, the border ring is not
        bad = CR.f(p, 0.7, y, act, True, defect=d)
        assert np.array_equal(bad[:, :, 1:-1, 1:-1], good[:, :, 1:-1, 1:-1]), d
        ring = np.abs(bad - good)
        ring[:, :, 1:-1, 1:-1] = np.inf
        if act != 'relu':                                 # (relu can be flat at a border pixel)
            assert float(ring.min()) > 0.0, d
        assert float(np.abs(bad - good).max()) > 1e-3, d
    # at t = 0 the time channel is zero everywhere: unclipped taps change nothing
    assert np.array_equal(CR.f(p, 0.0, y, act, True, defect='time_taps_unclipped'), CR.f(p, 0.0, y, act, True))
    # the last block of Fp = 32 holds input channel 16 alone: dropping it is zeroing that channel's conv2 weights
    q = [p[0], (p[1][0].copy(), p[1][1]), p[2]]
    q[1][0][:, 1 + 16] = 0.0
    assert np.array_equal(CR.f(p, 0.7, y, act, True, defect='drop_last_block'), CR.f(q, 0.7, y, act, True))
    with pytest.raises(AssertionError):
        CR.f(p, 0.7, y, act, True, defect='no_such_defect')


# ---------------------------------------------------------------------------------------------------------------------------------------
# evaluation cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_sees_every_filter_and_image_class():
    assert len(CC.INSTANTIATIONS) == 12 and len({c.name for c in CC.EVAL}) == len(CC.EVAL)
    for inst in CC.INSTANTIATIONS:
        mine = [c for c in CC.EVAL if (c.dtype, c.act, c.td) == inst]
        assert {c.F for c in mine} == set(CC.F_CLASSES), inst
        assert {(c.H, c.W) for c in mine} == set(CC.IMAGES), inst
    assert CC.F_CLASSES == (1, 15, 16, 17, 64, 113, 128) and CC.C_CLASSES == (1, 2, 15, 16) and CC.BATCHES == (1, 3, 257)
    assert set(CC.IMAGES) == {(1, 1), (1, 9), (9, 1), (8, 8), (8, 9), (9, 8), (16, 16), (17, 17), (7, 23)}
    for dtype in CC.DTYPES:
        mine = [c for c in CC.EVAL if c.dtype == dtype]
        assert {c.C for c in mine} == set(CC.C_CLASSES) and {c.B for c in mine} == set(CC.BATCHES), dtype
        assert any(c.C == 16 and c.F == 128 for c in CC.EVAL)                 # both maxima at once
    assert all((c.H, c.W) in ((1, 1), (8, 8)) for c in CC.EVAL if c.B == 257)
    assert all(c.B * c.H * c.W <= 600 for c in CC.EVAL if c.F >= 113)
    # what the classes are there for, in the kernel's terms
    assert [CC.n_blocks(F) for F in CC.F_CLASSES] == [1, 1, 1, 2, 4, 8, 8]
    assert [CC.n_tiles(*hw) for hw in CC.IMAGES] == [1, 2, 2, 1, 2, 2, 4, 9, 3]
    assert len(CC.BATCH_ROWS) >= 4 and {c.dtype for c in CC.BATCH_ROWS} == set(CC.DTYPES)


@pytest.mark.parametrize('case', CC.EVAL, ids=CC.ids(CC.EVAL))
def test_evaluation_case_has_size_and_power(case):
    """max |ref| >= 0.3, and each planted defect that applies deviates by at least ten float32 bounds (in the float32 measure)."""
    for t in CC.TIMES:
        ref, bound, pw = CC.reference(case, t), CC.f32_bound(case, t), CC.power(case, t)
        print('%s t %+.1f: max |ref| %.2f, E32 %.2e, bound %.2e, power %s' % (case.name, t, float(np.abs(ref).max()), CC.e32(case, t), bound,
                                                                            {k: '%.1e' % v for k, v in pw.items()}))
        assert ref.shape == (case.B, case.C, case.H, case.W) and np.isfinite(ref).all()
        assert float(np.abs(ref).max()) >= 0.3
        assert bands.case_ceiling(1, stages=3) * 4.0 <= bound < 1e-4
        assert set(pw) == ({'halo_is_act_b1', 'drop_last_block'} | ({'time_taps_unclipped'} if case.td else set()))
        for d, v in pw.items():
            assert v >= 10.0 * bound, (d, v, bound)


@pytest.mark.parametrize('case', CC.SATURATED, ids=CC.ids(CC.SATURATED))
def test_saturated_cases_saturate(case):
    for t in CC.TIMES:
        for z in CC.pre_activations(case, t):
            assert float((z > 20.0).mean()) >= 0.01 and float((z < -20.0).mean()) >= 0.01
        assert np.isfinite(CC.reference(case, t)).all() and CC.f32_bound(case, t) < 1e-4
    assert {(c.dtype, c.act) for c in CC.SATURATED} == {(d, a) for d in CC.DTYPES for a in ('softplus', 'tanh')}


def test_fixture_cases_have_the_shapes_they_are_there_for():
    for c in CC.STAGE.values():
        assert (c.H, c.W, c.B) == (17, 9, 3) and CC.n_tiles(c.H, c.W) == 6 and c.td
    assert CC.STAGE_NK == (0, 1, 7, 14) and max(CC.STAGE_NK) == N.MAX_STAGES + 1 == N.MAX_LINCOMB
    assert {(c.dtype, c.act) for c in CC.NONFINITE} == {(d, a) for d in CC.DTYPES for a in CC.ACTS}
    b, ch, py, px = CC.NONFINITE_AT
    for c in CC.NONFINITE:
        assert (c.B, c.H, c.W) == (3, 17, 17) and b == 1 and (py % CC.TILE, px % CC.TILE) == (7, 7) and py + 1 < c.H and px + 1 < c.W


# ---------------------------------------------------------------------------------------------------------------------------------------
# solve cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_solve_cases_cover_methods_dtypes_directions_and_activations():
    S = CC.ALL_SOLVES
    assert len({c.name for c in S}) == len(S)
    assert {c.method for c in S if c.dtype == 'float64'} == {'dopri5', 'tsit5', 'bosh3', 'adaptive_heun', 'dopri8'}
    assert {c.method for c in S if c.dtype == 'float32'} == {'dopri5', 'dopri8'}
    assert {c.t[-1] > c.t[0] for c in S} == {True, False} and {c.td for c in S} == {True, False}
    assert {c.act for c in S} == {'softplus', 'tanh', 'relu'} and sum(c.act == 'relu' for c in S) == 1
    assert all(c.B <= 3 and c.C <= 3 and c.H <= 9 and c.W <= 9 and c.F in (10, 17) and len(c.t) == 3 for c in S)
    assert {c.F for c in S} == {10, 17}
    assert len(CC.REJECTING) >= 3 and {w for c in CC.REJECTING for w in c.rejecting.split()} == {'first', 'after', 'covered'}
    assert all(not c.rejecting for c in CC.SOLVES) and all(c.options is None for c in S)


@pytest.mark.parametrize('case', CC.ALL_SOLVES, ids=CC.ids(CC.ALL_SOLVES))
def test_solve_case_is_admitted(case):
    hi = CC.oracle(case, 'float64')
    runs = [hi] + ([CC.oracle(case, 'float32')] if case.dtype == 'float32' else [])
    gap = min(abs(r - 1.0) for run in runs for r in run.ratios)
    sgn = 1.0 if case.t[-1] > case.t[0] else -1.0
    outs = [sgn * v for v in case.t[1:]]                 # output times in solver time (a decreasing axis is negated)
    span = abs(case.t[-1] - case.t[0])
    # every accepted step's end but the one that reaches the last output time, against every output time
    ends = [[row[0] + row[1] for row in run.trace if row[2]] for run in runs]
    near = min([abs(e - o) / span for es in ends for e in es[:-1] for o in outs] + [np.inf])
    print('%s: %s, %d attempts, %d accepted; ratio gap %.3f; nearest step boundary to an output time %.2e of the span; max |y| %.2f%s' % (
        case.name, CC.accepts(hi), hi.n_attempts, hi.n_accepted, gap, near, float(np.abs(hi.sol).max()),
        '; E32 %.2e, bound %.2e' % (CC.solve_e32(case), CC.solve_bound(case)) if case.dtype == 'float32' else ''))
    assert hi.sol.shape == (3, case.B, case.C, case.H, case.W) and all(np.isfinite(run.sol).all() for run in runs)
    assert len(hi.ratios) == hi.n_attempts >= 2 and hi.n_accepted >= 2
    assert gap > 0.02
    assert near > 1e-3
    for run in runs:
        assert [r <= 1.0 for r in run.ratios] == [bool(row[2]) for row in run.trace]
    if case.dtype == 'float32':
        lo = runs[1]
        assert CC.accepts(lo) == CC.accepts(hi) and lo.sol.dtype == np.float32
        assert 0.0 < CC.solve_bound(case) < 1e-3
    for run in runs:
        seq = CC.accepts(run)
        if 'first' in case.rejecting:
            assert seq.startswith('r'), seq
        if 'after' in case.rejecting:
            assert 'Ar' in seq, seq
        if 'covered' in case.rejecting:                  # a rejected attempt across the interior output time
            assert any(not row[2] and row[0] < outs[0] < row[0] + row[1] for row in run.trace), run.trace
        if not case.rejecting and case.method != 'tsit5':   # (the tsit5 case rejects at its plain scale: more of the same property)
            assert 'r' not in seq, seq


# ---------------------------------------------------------------------------------------------------------------------------------------
# mi_ode_conv_stage's refusals, through the C ABI: every one before the launch, one field wrong at a time
# ---------------------------------------------------------------------------------------------------------------------------------------
def _valid_call(n_k=2, td=1):
    """A descriptor and arguments that pass every check (the pointers are host buffers that nothing dereferences before the launch)."""
    buf = (C.c_double * 8)()
    ptr = C.addressof(buf)
    d = N.ConvDesc()
    d.dtype, d.activation, d.time_dependent, d.sign = N.F64, N.CONV_ACT_TANH, td, 1.0
    d.batch, d.channels, d.height, d.width, d.filters = 2, 3, 9, 9, 17
    d.w1 = d.b1 = d.w2 = d.w2t = d.b2 = d.w3 = d.b3 = ptr
    ks = (C.c_void_p * 16)(*([ptr] * 16))
    beta = (C.c_double * 16)(*([0.5] * 16))
    args = dict(y0=ptr, ks=ks, n_k=n_k, beta=beta, dt=ptr, t=ptr, k_out=ptr, y_out=None)
    return d, args, buf


def _refused(d, a):
    lib = N.load()
    rc = lib.mi_ode_conv_stage(C.byref(d) if d is not None else None, a['y0'], a['ks'], a['n_k'], a['beta'], a['dt'], a['t'], a['k_out'], a['y_out'], None)
    return rc, N.last_error()


REFUSALS = [
    ('channels-0', lambda d, a: setattr(d, 'channels', 0), 'channels'),
    ('channels-17', lambda d, a: setattr(d, 'channels', 17), 'channels'),
    ('filters-0', lambda d, a: setattr(d, 'filters', 0), 'filters'),
    ('filters-129', lambda d, a: setattr(d, 'filters', 129), 'filters'),
    ('batch-0', lambda d, a: setattr(d, 'batch', 0), 'empty batch'),
    ('height-0', lambda d, a: setattr(d, 'height', 0), 'empty batch'),
    ('dtype', lambda d, a: setattr(d, 'dtype', 7), 'bad dtype'),
    ('activation', lambda d, a: setattr(d, 'activation', 3), 'bad activation'),
    ('td-null-w2t', lambda d, a: setattr(d, 'w2t', None), 'null weight'),
    ('td-null-t', lambda d, a: a.update(t=None), 'null weight'),
    ('null-w3', lambda d, a: setattr(d, 'w3', None), 'null weight'),
    ('n_k-15', lambda d, a: a.update(n_k=15), 'n_k 15'),
    ('n_k-negative', lambda d, a: a.update(n_k=-1), 'n_k -1'),
    ('null-ks', lambda d, a: a.update(ks=None), 'bad stage combination'),
    ('null-beta', lambda d, a: a.update(beta=None), 'bad stage combination'),
    ('null-dt', lambda d, a: a.update(dt=None), 'bad stage combination'),
    ('null-k1', lambda d, a: a['ks'].__setitem__(1, None), 'null k[1]'),
    ('null-y0', lambda d, a: a.update(y0=None), 'null descriptor'),
    ('null-k_out', lambda d, a: a.update(k_out=None), 'null descriptor'),
]


@pytest.mark.parametrize('name,spoil,why', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_conv_stage_refuses_one_wrong_field(name, spoil, why):
    d, a, keep = _valid_call()
    spoil(d, a)
    rc, msg = _refused(d, a)
    assert rc < 0 and 'conv_stage' in msg and why in msg, (rc, msg)


def test_conv_stage_limits_are_the_headers():
    assert (N.CONV_MAX_C, N.CONV_MAX_F, N.MAX_STAGES + 1) == (16, 128, 14)
    d, a, keep = _valid_call()
    rc, msg = _refused(None, a)
    assert rc < 0 and 'null descriptor' in msg
    # a time-independent descriptor needs neither w2t nor t: with both null the call is refused for the NEXT wrong field, not for them
    d, a, keep = _valid_call(td=0)
    d.w2t = None
    a.update(t=None)
    d.activation = 9
    rc, msg = _refused(d, a)
    assert rc < 0 and 'bad activation' in msg, msg
    # n_k = 14 passes the stage-combination check (it is the maximum): the refusal is the later one
    d, a, keep = _valid_call(n_k=14)
    d.activation = 9
    rc, msg = _refused(d, a)
    assert rc < 0 and 'bad activation' in msg, msg
