"""The fused convolutional stage kernel (csrc/mi_ode_conv.h: k_conv_stage<T, ACT, TD>; csrc/mi_ode_conv.hip; rhs.Conv2dODE;
Conv2dODEFunc.device_rhs) at its edges on the MI355X, against the float64 numpy restatement (tests/conv_restatement.py) and the numpy oracle
(oracle/ode_numpy.py) on the cases of tests/conv_cases.py - whose properties (coverage, size, power against three planted defects,
saturation, admission of the solves) tests/test_conv_cases_host.py asserts on the CPU.

Bars.  float64: max |got - ref| / max(1, max |ref|) <= 1e-12.  float32: bands.observed(got, ref) <= 4 x max(E32, bands.case_ceiling(n,
stages)), ref the float64 restatement (oracle run) on the float32-rounded inputs and E32 the float32 restatement's (oracle run's) own
deviation from it.  Nothing measured on the kernel enters a bound."""
import numpy as np
import pytest
import torch

from tests import bands
from tests import conv_cases as CC
from tests import conv_restatement as CR
from tfdiffeq_amd import models, odeint
from tfdiffeq_amd.misc import _DevScalar, _lincomb

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TD = {'float64': torch.float64, 'float32': torch.float32}


def _desc(case, dtype=None):
    fn = CC.module(case).to(DEV, TD[dtype or case.dtype])
    return fn, fn.device_rhs()


def _dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(DEV, TD[dtype])          # (a writable copy: the cached inputs are read only)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


def _same(a, b):
    """Bit-identical up to the payload of a NaN (torch.equal is False wherever a NaN is)."""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _hold(case, got, ref, bound32, what):
    """One comparison at the case's bar; prints the figure before it asserts."""
    got = got.double().cpu().numpy()
    if case.dtype == 'float64':
        obs, bar = _rel(got, ref), CC.F64_BAR
    else:
        obs, bar = bands.observed(got, ref), bound32
    print('%s %s: observed %.3e, bar %.3e' % (case.name, what, obs, bar))
    assert obs <= bar, (case.name, what, obs, bar)


def _evaluate(case):
    fn, desc = _desc(case)
    y = _dev(CC.state(case), case.dtype)
    outs = []
    for i, t in enumerate(CC.TIMES):
        tt = torch.tensor(t, dtype=TD[case.dtype], device=DEV)
        with torch.no_grad():
            got = desc(tt, y)
            if i == 1:                                   # a reversed axis: -f(-t, y), the sign folded into the kernel
                assert torch.equal(desc.reversed()(-tt, y), -got)
        _hold(case, got, CC.reference(case, t), CC.f32_bound(case, t), 't %+.1f' % t)
        outs.append(got)
    return desc, y, outs


@pytest.mark.parametrize('case', CC.EVAL, ids=CC.ids(CC.EVAL))
def test_evaluation_matches_restatement(case):
    _evaluate(case)


@pytest.mark.parametrize('case', CC.SATURATED, ids=CC.ids(CC.SATURATED))
def test_saturated_activations_match_restatement(case):
    _evaluate(case)


@pytest.mark.parametrize('case', CC.BATCH_ROWS, ids=CC.ids(CC.BATCH_ROWS))
def test_images_are_independent_and_calls_repeat(case):
    """f(y)[i] is bit-identical to f(y[i:i+1]) for the first and the last image (the tile map depends on the image alone), and two calls agree."""
    desc, y, outs = _evaluate(case)
    tt = torch.tensor(CC.TIMES[0], dtype=y.dtype, device=DEV)
    with torch.no_grad():
        assert torch.equal(desc(tt, y), outs[0])
        for i in (0, case.B - 1):
            assert torch.equal(desc(tt, y[i:i + 1]), outs[0][i:i + 1]), i


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage()
# ---------------------------------------------------------------------------------------------------------------------------------------
def _stage_inputs(dtype, n_k):
    case = CC.STAGE[dtype]
    rng = np.random.default_rng(11 + n_k)
    y0 = _dev(CC.state(case), dtype)
    ks = [_dev(rng.standard_normal(CC.state(case).shape), dtype) for _ in range(n_k)]
    beta = [float(v) for v in rng.uniform(-1.0, 1.0, n_k)]
    return case, y0, ks, beta


def _check_stage(desc, t, y0, ks, beta, dt, want_y=True):
    k, ys = desc.stage(t, y0, ks, beta, dt, want_y=want_y)
    ref = _lincomb(y0, beta, ks, dt) if ks else y0.contiguous()
    if want_y:
        assert _same(ys, ref)
    else:
        assert ys is None
    with torch.no_grad():
        assert _same(k, desc(t, ref))
    return k, ys


@pytest.mark.parametrize('n_k', CC.STAGE_NK)
@pytest.mark.parametrize('dtype', CC.DTYPES)
def test_stage_state_is_lincomb_and_k_is_the_evaluation(dtype, n_k):
    case, y0, ks, beta = _stage_inputs(dtype, n_k)
    fn, desc = _desc(case)
    t = torch.tensor(0.4, dtype=TD[dtype], device=DEV)
    dt = torch.tensor(0.137, dtype=torch.float64, device=DEV)
    k, ys = _check_stage(desc, t, y0, ks, beta, dt)
    k2, none = _check_stage(desc, t, y0, ks, beta, dt, want_y=False)
    assert torch.equal(k, k2)
    with torch.no_grad():                                # ... and the evaluation itself is the restatement's, on the kernel's own y_s
        ref = CR.f(list(CC.params(case)), 0.4, ys.double().cpu().numpy(), case.act, case.td)
    _hold(case, k, ref, 4.0 * bands.case_ceiling(1, stages=3), 'stage n_k %d' % n_k)


@pytest.mark.parametrize('dtype', CC.DTYPES)
def test_stage_variants(dtype):
    case, y0, ks, beta = _stage_inputs(dtype, 7)
    fn, desc = _desc(case)
    t = torch.tensor(-0.4, dtype=TD[dtype], device=DEV)
    dt = torch.tensor(0.137, dtype=torch.float64, device=DEV)
    base_k, base_y = _check_stage(desc, t, y0, ks, beta, dt)
    assert bool(torch.isfinite(base_k).all())
    # a zero beta entry against a k_j that holds a NaN: 0 x NaN = NaN in _lincomb, and in the kernel
    beta0 = list(beta)
    beta0[3] = 0.0
    ks_nan = list(ks)
    ks_nan[3] = ks[3].clone()
    ks_nan[3][1, 2, 8, 7] = float('nan')                 # (pixel (8, 7): first row of the last tile row, last column of the first tile)
    k, ys = _check_stage(desc, t, y0, ks_nan, beta0, dt)
    assert bool(ys[1, 2, 8, 7].isnan()) and int(ys.isnan().sum()) == 1
    assert not bool(k[0].isnan().any()) and not bool(k[2].isnan().any()) and bool(k[1].isnan().any())
    # negative dt
    ndt = torch.tensor(-0.05, dtype=torch.float64, device=DEV)
    k, ys = _check_stage(desc, t, y0, ks, beta, ndt)
    assert not torch.equal(ys, base_y)
    # dt as a misc._DevScalar (a float64 in device memory that is not a tensor)
    k, ys = _check_stage(desc, t, y0, ks, beta, _DevScalar(dt.data_ptr()))
    assert torch.equal(k, base_k) and torch.equal(ys, base_y)
    # channels-last ks and y0, and y0 a strided batch slice: bit-identical to the contiguous copies
    cl = [x.contiguous(memory_format=torch.channels_last) for x in ks]
    assert not cl[0].is_contiguous()
    k, ys = desc.stage(t, y0.contiguous(memory_format=torch.channels_last), cl, beta, dt, want_y=True)
    assert torch.equal(k, base_k) and torch.equal(ys, base_y) and k.is_contiguous() and ys.is_contiguous()
    wide = torch.empty(2 * y0.shape[0], *y0.shape[1:], dtype=y0.dtype, device=DEV).fill_(float('nan'))
    wide[::2] = y0
    assert not wide[::2].is_contiguous()
    k, ys = desc.stage(t, wide[::2], ks, beta, dt, want_y=True)
    assert torch.equal(k, base_k) and torch.equal(ys, base_y)
    with torch.no_grad():
        assert torch.equal(desc(t, wide[::2]), desc(t, y0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# non-finite values
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', CC.NONFINITE, ids=CC.ids(CC.NONFINITE))
def test_non_finite_pixel_stays_in_its_neighbourhood(case, value):
    fn, desc = _desc(case)
    b, ch, py, px = CC.NONFINITE_AT
    y_np = CC.state(case).copy()
    clean = _dev(y_np, case.dtype)
    y_np[b, ch, py, px] = value
    bad = _dev(y_np, case.dtype)
    t = CC.TIMES[0]
    tt = torch.tensor(t, dtype=TD[case.dtype], device=DEV)
    with torch.no_grad():
        got_clean = desc(tt, clean)
        got = desc(tt, bad)
    with np.errstate(all='ignore'):
        ref = CR.f(list(CC.params(case)), t, y_np, case.act, case.td)
    near = np.zeros(ref.shape, dtype=bool)               # the 3 x 3 neighbourhood, across four tiles, every channel of that image only
    near[b, :, py - 1:py + 2, px - 1:px + 2] = True
    got_np = got.double().cpu().numpy()
    assert np.array_equal(~np.isfinite(got_np), ~np.isfinite(ref))
    assert not (~np.isfinite(ref) & ~near).any()
    if np.isnan(value):
        assert np.array_equal(np.isnan(got_np), near)
    # every element outside the neighbourhood is bit-identical to the clean run; the finite ones inside are the restatement's
    assert torch.equal(got[torch.from_numpy(~near).to(DEV)], got_clean[torch.from_numpy(~near).to(DEV)])
    fin = near & np.isfinite(ref)
    if fin.any():
        bar = CC.F64_BAR if case.dtype == 'float64' else CC.f32_bound(case, t)
        obs = float((np.abs(got_np[fin] - ref[fin]) / (1.0 + np.abs(ref[fin]))).max())
        print('%s: finite neighbours of the poisoned pixel: observed %.3e, bar %.3e' % (case.name, obs, bar))
        assert obs <= bar
    # then a clean call on the same descriptor is still correct
    with torch.no_grad():
        again = desc(tt, clean)
    assert torch.equal(again, got_clean)
    _hold(case, again, CC.reference(case, t), CC.f32_bound(case, t), 'clean call after the poisoned one')


# ---------------------------------------------------------------------------------------------------------------------------------------
# dtype crossing and stale weights
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('module_dtype,state_dtype', [('float64', 'float32'), ('float32', 'float64')])
def test_state_dtype_differs_from_the_modules_and_weights_change_in_place(module_dtype, state_dtype):
    """The case's weights and state are genuine float64 values: a float64 module with a float32 state has its weights ROUNDED by DeviceRHS._dev
    (and a float32 module rounds them itself) - the target is the restatement on the float32-rounded weights and the state as the kernel got it."""
    case = CC.CROSSING
    fn = CC.module(case)
    with torch.no_grad():                                # (torch initialises in float32: x (1 + 2^-30) leaves no weight float32-representable)
        for p_ in fn.parameters():
            p_.mul_(1.0 + 2.0 ** -30)
    w2 = CR.params(fn)[1][0]
    assert case.dtype == 'float64' and float((w2 != w2.astype(np.float32)).mean()) > 0.99
    fn = fn.to(DEV, TD[module_dtype])
    y = _dev(CC.state(case), state_dtype)
    y_np = y.double().cpu().numpy()
    t = CC.TIMES[0]
    tt = torch.tensor(t, dtype=TD[state_dtype], device=DEV)
    as_state = case._replace(dtype=state_dtype, name='%s-module-%s-state-%s' % (case.name, module_dtype, state_dtype))

    def check(what):
        with torch.no_grad():
            got = fn.device_rhs()(tt, y)
        assert got.dtype == TD[state_dtype]
        p = [(W.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)) for W, b in CR.params(fn)]
        ref = CR.f(p, t, y_np, case.act, case.td)
        e32 = bands.observed(CR.f32(p, t, y_np, case.act, case.td), ref)
        _hold(as_state, got, ref, 4.0 * max(e32, bands.case_ceiling(1, stages=3)), what)
        return got
    first = check('first call')
    again = check('second call (the converted copies come from the cache)')
    assert torch.equal(first, again)
    with torch.no_grad():                                # a hand-written optimizer step: .data bumps no version counter of the parameter
        fn.conv2.weight.data -= 0.5
        fn.conv1.bias.data += 0.1
    second = check('after the in-place update')
    assert not torch.equal(first, second) and float((first - second).abs().max()) > 1e-2


@pytest.mark.parametrize('dtype', CC.DTYPES)
def test_odeblock_inference_sees_an_optimizer_step(dtype):
    """Inference, optimizer.step(), inference again through models.ODEBlock(is_conv=True): each against the oracle solve with the weights of
    that moment (the descriptor's copies are refreshed in place, nothing cached on them goes stale), with the oracle's attempt counts.
    float64 at tol 1e-6 to 1e-9; float32 at tol 1e-4 (truncation error steers the controller) to the float32 solve bound."""
    from oracle import ode_numpy as O
    case = CC.Eval(dtype, 'tanh', True, 2, 3, 9, 9, 17, seed=4, prefix='odeblock')
    tol = 1e-6 if dtype == 'float64' else 1e-4
    fn = CC.module(case).to(DEV, TD[dtype])
    block = models.ODEBlock(fn, is_conv=True, tol=tol)
    x = _dev(CC.state(case) * 0.5, dtype)
    x_np = x.double().cpu().numpy()
    opt = torch.optim.SGD(fn.parameters(), lr=0.05)

    def oracle(rhs, y0):
        return O.odeint(rhs, y0, np.array([0., 1.]), rtol=tol, atol=tol, method='dopri5', return_stats=True)

    def check(what):
        with torch.no_grad():
            got = block(x)
        st = dict(odeint.last_stats)
        assert 'fused stage kernel' in st['engine'] and st['python_evaluations'] == 0
        p = CR.params(fn)
        ref, hi = oracle(lambda t_, y_: CR.f(p, t_, y_, case.act, case.td), x_np)
        if dtype == 'float64':
            own, bound = hi, None
        else:
            lo, own = oracle(lambda t_, y_: CR.f32(p, t_, y_, case.act, case.td), x_np.astype(np.float32))
            bound = 4.0 * max(bands.observed(lo[1], ref[1]), bands.case_ceiling(own.n_attempts, stages=7))
        print('%s %s: attempts / accepted %s, oracle %s' % (case.name, what, (st['n_attempts'], st['n_accepted']), (own.n_attempts, own.n_accepted)))
        assert (st['n_attempts'], st['n_accepted']) == (own.n_attempts, own.n_accepted)
        if dtype == 'float64':
            obs = _rel(got.cpu().numpy(), ref[1])
            print('%s %s: observed %.3e, bar 1e-9' % (case.name, what, obs))
            assert obs <= 1e-9
        else:
            _hold(case, got, ref[1], bound, what)
        return got
    first = check('before the step')
    for p_ in fn.parameters():
        p_.grad = torch.full_like(p_, 0.5)
    opt.step()
    second = check('after optimizer.step()')
    assert float((first - second).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole solves against the numpy oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
def _solve(case, graph):
    fn, desc = _desc(case)
    y0 = _dev(CC.solve_state(case), case.dtype)
    with torch.no_grad():
        got = odeint(desc, y0, torch.tensor(case.t, dtype=torch.float64), rtol=case.rtol, atol=case.atol, method=case.method,
                     options=dict({'graph': graph}, **({'first_step': case.first_step} if case.first_step else {})))
    return got, dict(odeint.last_stats)


@pytest.mark.parametrize('case', CC.ALL_SOLVES, ids=CC.ids(CC.ALL_SOLVES))
def test_solve_takes_the_oracles_steps(case):
    got, st = _solve(case, False)
    assert 'fused stage kernel' in st['engine'] and st['python_evaluations'] == 0, st
    run = CC.oracle(case, case.dtype)
    counts = (st.get('n_attempts'), st.get('n_accepted'), st.get('n_rejected'))
    print('%s: attempts / accepted / rejected %s, oracle %s' % (case.name, counts, (run.n_attempts, run.n_accepted, run.n_attempts - run.n_accepted)))
    assert counts == (run.n_attempts, run.n_accepted, run.n_attempts - run.n_accepted)
    ref = CC.oracle(case, 'float64').sol
    if case.dtype == 'float64':
        obs, bar = _rel(got.cpu().numpy(), ref), (1e-8 if case.act == 'relu' else 1e-9)
        print('%s: observed %.3e, bar %.1e' % (case.name, obs, bar))
        assert obs <= bar
    else:
        _hold(case, got, ref, CC.solve_bound(case), 'E32 %.2e' % CC.solve_e32(case))
    if case.method == 'dopri5':
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            rec, st_g = _solve(case, True)
        assert 'hipGraph' in st_g['engine'] and st_g['python_evaluations'] == 0, st_g
        assert torch.equal(rec, got)
