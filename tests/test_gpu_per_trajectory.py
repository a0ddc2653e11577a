"""Per-trajectory step control on the GPU (options={'per_trajectory': True}; csrc/mi_ode_rows.h, k_rows_rowlocal): row i of a call is what
`odeint(func, y0[i:i+1], t, ...)` returns on the existing shared kernel - bit for bit, with that call's counts - and what the oracle computes
for that row alone.

Inputs.  The base input is the issue's: 70 Lorenz rows spread over 3.3 decades, t = linspace(0, 1, 5), rtol 1e-6, atol 1e-9, dopri5 (oracle
attempts per row 39 .. 50, shared control 56).  The other methods run Lotka-Volterra with nine spread rows (tests/per_trajectory_cases.py
`lv_y0`) at tolerances the oracle needs 4 .. 150 attempts per row for (all 5 methods x 9 rows: under a second on the CPU).  float32 runs use
rtol 1e-4 / atol 1e-6, as the existing float32 tests do.

Tolerances.  Against a batch-1 call: torch.equal.  Against the oracle, float64: counts exactly (tsit5: the three attempts
tests/test_gpu_parity.py allows the corrected tableau) and the band of tests/test_gpu_parity.py (rtol 1e-5, atol 1e-6).  float32: the
oracle runs in float32 too (the state dtype, as the reference does); counts within max(2, attempts // 20) (tests/test_gpu_parity.py); the
state within `f32_ceiling`: the rule the existing suite applies to a float32 run held to the oracle on inputs that are no golden fixture
(tests/test_gpu_round5.py: max(2e-4, bands.case_ceiling(attempts)) - two float32 solves at rtol 1e-4 whose step sequences fork on one
rounding differ by the solve's own tolerance, 2 x rtol, whatever the roundoff bound says), under the 1e-3 (dopri8: 3e-3) ceiling of
tests/bands.py / tests/test_gpu_parity.py for the row-local kernels.  (A first version of this file held these rows to
bands.case_ceiling(attempts, stages, growth = 1) alone - the formula of the golden fixtures, whose `attempts` is the reference trace's -
with the oracle in float64: Lotka-Volterra dopri5 float32, row 4, 9 attempts: observed 3.06e-5 against 3.00e-5.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_trajectory_cases as PC                          # noqa: E402
from oracle import ode_numpy as O                         # noqa: E402
from tests.bands import case_ceiling, observed            # noqa: E402
from tfdiffeq_amd import _native as N                     # noqa: E402
from tfdiffeq_amd import odeint, rhs                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
TOL = {F64: dict(rtol=1e-6, atol=1e-9), F32: dict(rtol=1e-4, atol=1e-6)}
ENGINE = 'k_rows_rowlocal: per-trajectory step control, one launch'


def rows_call(f, y0, t, method='dopri5', tol=None, **opts):
    sol = odeint(f, y0, torch.as_tensor(t), method=method, options=dict(opts, per_trajectory=True), **(tol or TOL[y0.dtype]))
    st = dict(odeint.last_stats)
    assert st['engine'] == ENGINE and st['n_launches'] == 1 and st['per_trajectory'] is True and st['status'] == 0, st
    r = st['rows']
    assert all(r[k].shape == (y0.shape[0],) and r[k].is_cuda for k in ('n_attempts', 'n_accepted', 'nfe', 'status'))
    assert (st['n_attempts'], st['n_accepted'], st['nfe']) == (int(r['n_attempts'].max()), int(r['n_accepted'].max()), int(r['nfe'].max()))
    return sol, st


def one_call(f, y0, i, t, method='dopri5', tol=None, **opts):
    """The definition: the existing shared kernel on row i alone."""
    sol = odeint(f, y0[i:i + 1], torch.as_tensor(t), method=method, options=opts, **(tol or TOL[y0.dtype]))
    st = dict(odeint.last_stats)
    assert st.get('per_trajectory') is None and st['n_launches'] == 1, st
    return sol, st


def assert_row_is_the_batch_one_call(sol, st, f, y0, i, t, method='dopri5', tol=None, **opts):
    ref, rs = one_call(f, y0, i, t, method, tol, **opts)
    assert torch.equal(sol[:, i], ref[:, 0]), (method, i, float((sol[:, i] - ref[:, 0]).abs().max()))
    got = tuple(int(st['rows'][k][i]) for k in ('n_attempts', 'n_accepted', 'nfe', 'status'))
    assert got == (rs['n_attempts'], rs['n_accepted'], rs['nfe'], 0), (method, i, got, rs)


_ORACLE = {}


def oracle_rows(key, f_np, y0, t, method, tol, options=None):
    """The oracle on every row alone, computed once per input and shared."""
    if key not in _ORACLE:
        sols, counts = [], []
        for i in range(y0.shape[0]):
            ref, st = O.odeint(f_np, y0[i:i + 1], np.asarray(t), method=method, options=options, return_stats=True, **tol)
            sols.append(ref[:, 0])
            counts.append((st.n_attempts, st.n_accepted))
        _ORACLE[key] = (np.stack(sols, axis=1), counts)
    return _ORACLE[key]


def band64(got, ref, what):
    bad = np.abs(got - ref) > 1e-6 + 1e-5 * np.abs(ref)
    assert not bad.any(), '%s: %d/%d outside band, max abs diff %.3e' % (what, bad.sum(), bad.size, np.abs(got - ref).max())


def f32_ceiling(attempts, stages, growth=1.0, method='dopri5'):
    if method == 'dopri8':                                # tests/bands.py: cancellation in the 13-stage combination in float32 - its own ceiling
        return 3e-3
    return min(1e-3, max(2e-4, case_ceiling(attempts, stages, growth)))


def base(dtype):
    return PC.base_y0().to(device=DEV, dtype=dtype)


# ---- the row definition ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32])
def test_rows_are_the_batch_one_calls_bit_for_bit(dtype):
    y0 = base(dtype)
    sol, st = rows_call(rhs.Lorenz(), y0, PC.BASE_T)
    assert sol.shape == (5, 70, 3) and sol.dtype == dtype and torch.equal(sol[0], y0)
    for i in PC.BASE_ROWS:
        assert_row_is_the_batch_one_call(sol, st, rhs.Lorenz(), y0, i, PC.BASE_T)


@pytest.mark.parametrize('dtype', [F64, F32])
def test_every_row_against_the_oracle(dtype):
    y0 = base(dtype)
    sol, st = rows_call(rhs.Lorenz(), y0, PC.BASE_T)
    ref, counts = oracle_rows(('lorenz', dtype), PC.lorenz_np, y0.cpu().numpy(), PC.BASE_T, 'dopri5', TOL[dtype])       # (the oracle in the state dtype)
    att, acc = st['rows']['n_attempts'].cpu().tolist(), st['rows']['n_accepted'].cpu().tolist()
    got = sol.cpu().numpy()
    if dtype == F64:
        assert list(zip(att, acc)) == counts, [(i, a, c) for i, (a, c) in enumerate(zip(zip(att, acc), counts)) if a != c]
        assert [counts[i][0] for i in PC.BASE_ROWS] == [50, 47, 46, 43, 42, 39]
        band64(got, ref, 'lorenz dopri5 float64')
    else:
        for i, (a, (ra, _)) in enumerate(zip(att, counts)):
            assert abs(a - ra) <= max(2, ra // 20), (i, a, ra)
            obs, ceil = observed(got[:, i], ref[:, i]), f32_ceiling(ra, 7, float(np.exp(0.9)))
            print('row %d: %d attempts (oracle %d), observed %.2e, ceiling %.2e' % (i, a, ra, obs, ceil))
            assert obs <= ceil, (i, obs, ceil)


def test_the_distinction_cannot_collapse():
    y0 = base(F64)
    sol, st = rows_call(rhs.Lorenz(), y0, PC.BASE_T)
    shared = odeint(rhs.Lorenz(), y0, torch.as_tensor(PC.BASE_T), method='dopri5', **TOL[F64])
    ss = dict(odeint.last_stats)
    att = st['rows']['n_attempts']
    assert int(att.min()) < int(att.max()) and ss['n_attempts'] == 56 and ss.get('per_trajectory') is None, (att, ss)
    assert st['n_attempts'] == int(att.max()) < ss['n_attempts']
    differs = [i for i in range(70) if not torch.equal(sol[:, i], shared[:, i])]
    assert len(differs) >= 1
    off = odeint(rhs.Lorenz(), y0, torch.as_tensor(PC.BASE_T), method='dopri5', options={'per_trajectory': False}, **TOL[F64])
    assert torch.equal(off, shared) and odeint.last_stats['n_attempts'] == 56         # False is today's call, bit for bit


# ---- every method ------------------------------------------------------------------------------------------------------------------------------
LV_CASES = {      # method -> (t, float64 tolerances, oracle options, stages per attempt)
    'dopri5': (np.linspace(0., 2., 5), dict(rtol=1e-6, atol=1e-9), None, 7),
    'tsit5': (np.linspace(0., 2., 5), dict(rtol=1e-6, atol=1e-9), {'tsit5_fixed': True}, 7),
    'bosh3': (np.linspace(0., .5, 5), dict(rtol=1e-4, atol=1e-7), None, 4),
    'dopri8': (np.linspace(0., 2., 5), dict(rtol=1e-6, atol=1e-9), None, 14),
    'adaptive_heun': (np.linspace(0., 1., 5), dict(rtol=1e-3, atol=1e-6), None, 2),
}


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('method', sorted(LV_CASES))
def test_every_method_against_the_oracle_per_row(method, dtype):
    t, tol64, oopts, stages = LV_CASES[method]
    tol = tol64 if dtype == F64 else dict(rtol=max(tol64['rtol'], 1e-4), atol=max(tol64['atol'], 1e-6))
    y0 = PC.lv_y0().to(device=DEV, dtype=dtype)
    sol, st = rows_call(rhs.LotkaVolterra(), y0, t, method, tol)
    ref, counts = oracle_rows(('lv', method, dtype), PC.lv_np, y0.cpu().numpy(), t, method, tol, oopts)                # (the oracle in the state dtype)
    att, acc = st['rows']['n_attempts'].cpu().tolist(), st['rows']['n_accepted'].cpu().tolist()
    got = sol.cpu().numpy()
    assert len(set(att)) > 1, att
    for i, ((a, c), (ra, rc)) in enumerate(zip(zip(att, acc), counts)):
        if dtype == F64:
            if method == 'tsit5':
                assert abs(a - ra) <= 3, (i, a, ra)
            else:
                assert (a, c) == (ra, rc), (i, a, c, ra, rc)
        else:
            assert abs(a - ra) <= max(2, ra // 20), (i, a, ra)
    if dtype == F64:
        band64(got, ref, 'lv %s float64' % method)
    else:
        for i, (ra, _) in enumerate(counts):
            ceil = f32_ceiling(ra, stages, 1.0, method)
            obs = observed(got[:, i], ref[:, i])
            print('%s row %d: observed %.2e, ceiling %.2e' % (method, i, obs, ceil))
            assert obs <= ceil, (method, i, obs, ceil)
    for i in (0, 8):                                        # ... and the row definition, for every instantiation
        assert_row_is_the_batch_one_call(sol, st, rhs.LotkaVolterra(), y0, i, t, method, tol)


# ---- dense output and the time axis ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['50_outputs', '3_outputs', 'decreasing', 'first_step', 'tsit5_50_outputs'])
def test_dense_output_and_time_axis(case):
    f, y0, rows = rhs.Lorenz(), base(F64), (3, 66)
    method, opts = 'dopri5', {}
    t = {'50_outputs': np.linspace(0., 1., 50), '3_outputs': np.array([0., 1.5, 3.0]), 'decreasing': np.linspace(1., 0.4, 7),
         'first_step': PC.BASE_T, 'tsit5_50_outputs': np.linspace(0., 1., 50)}[case]
    if case == 'first_step':
        opts = {'first_step': 1e-3}
    if case.startswith('tsit5'):
        method = 'tsit5'
    if case.endswith('50_outputs'):
        # several outputs per step: Lotka-Volterra (the oracle accepts 13 .. 15 dopri5 steps over [0, 2] on these rows; Lorenz needs as
        # many steps over [0, 1] as there are outputs)
        f, y0, rows = rhs.LotkaVolterra(), PC.lv_y0().to(DEV), (0, 8)
    sol, st = rows_call(f, y0, t, method, **opts)
    assert sol.shape == (len(t),) + tuple(y0.shape)
    for i in rows:
        assert_row_is_the_batch_one_call(sol, st, f, y0, i, t, method, **opts)
    if case == '3_outputs':
        assert int(st['rows']['n_accepted'].min()) > 20              # many steps per output
    if case.endswith('50_outputs'):
        assert 3 * int(st['rows']['n_accepted'].max()) <= 49         # at least three outputs per step on every row


def test_more_output_times_than_the_lds_stage_holds():
    y0 = base(F64)[:5]
    t = np.linspace(0., 0.5, 1030)
    sol, st = rows_call(rhs.Lorenz(), y0, t)
    assert_row_is_the_batch_one_call(sol, st, rhs.Lorenz(), y0, 4, t)


# ---- batch edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', [1, 64, 65, 256, 257, 256 * 3 + 5])
def test_batch_edges(batch):
    reps = -(-batch // 70)
    y0 = base(F64).repeat(reps, 1)[:batch].contiguous()
    y0 = y0 * (1 + 1e-3 * torch.arange(batch, device=DEV, dtype=F64))[:, None]           # (no two rows alike)
    sol, st = rows_call(rhs.Lorenz(), y0, PC.BASE_T)
    assert sol.shape == (5, batch, 3) and torch.isfinite(sol).all()
    for i in sorted({0, batch // 2, max(batch - 2, 0), batch - 1, min(63, batch - 1), min(64, batch - 1), min(255, batch - 1), min(256, batch - 1)}):
        assert_row_is_the_batch_one_call(sol, st, rhs.Lorenz(), y0, i, PC.BASE_T)


def test_whole_wavefronts_that_finish_early():
    """Rows 0 .. 63 sit next to the Lotka-Volterra fixed point (oracle: 9 attempts), rows 64 .. 127 away from it (19): the first wavefront is
    done when the second is half way."""
    g = torch.Generator().manual_seed(3)
    jitter = 1e-3 * torch.randn(128, 2, generator=g, dtype=F64)
    y0 = (torch.cat([torch.tensor([[3.1, 1.5]], dtype=F64).repeat(64, 1), torch.tensor([[5., 5.]], dtype=F64).repeat(64, 1)]) + jitter).to(DEV)
    t = np.linspace(0., 2., 5)
    sol, st = rows_call(rhs.LotkaVolterra(), y0, t)
    att = st['rows']['n_attempts'].cpu()
    for i in (0, 63, 64, 127):
        _, rs = O.odeint(PC.lv_np, y0[i:i + 1].cpu().numpy(), t, method='dopri5', return_stats=True, **TOL[F64])
        assert int(att[i]) == rs.n_attempts
        assert_row_is_the_batch_one_call(sol, st, rhs.LotkaVolterra(), y0, i, t)
    ratio = float(att[:64].double().mean() / att[64:].double().mean())
    assert int(att[:64].max()) < int(att[64:].min()) and 0.35 <= ratio <= 0.65, (att, ratio)


# ---- plugins and lowered callables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32])
def test_custom_row_local_plugin(dtype):
    vdp = PC.van_der_pol()
    g = torch.Generator().manual_seed(5)
    y0 = (torch.randn(70, 2, generator=g, dtype=F64) * (10 ** torch.linspace(-1.5, 0.5, 70, dtype=F64))[:, None]).to(device=DEV, dtype=dtype)
    t = np.linspace(0., 1., 4)
    sol, st = rows_call(vdp, y0, t)
    assert int(st['rows']['n_attempts'].min()) < int(st['rows']['n_attempts'].max())
    for i in (0, 40, 69):
        assert_row_is_the_batch_one_call(sol, st, vdp, y0, i, t)
    if dtype == F64:
        ref, counts = oracle_rows(('vdp', dtype), PC.vdp_np, y0.cpu().numpy(), t, 'dopri5', TOL[F64])
        assert list(zip(st['rows']['n_attempts'].cpu().tolist(), st['rows']['n_accepted'].cpu().tolist())) == counts
        band64(sol.cpu().numpy(), ref, 'van der Pol plugin')


@pytest.mark.parametrize('dtype', [F64, F32])
def test_lowered_python_callable(dtype):
    g = torch.Generator().manual_seed(6)
    y0 = (torch.randn(70, PC.TIME_DIM, generator=g, dtype=F64) * (10 ** torch.linspace(-2, 1, 70, dtype=F64))[:, None]).to(device=DEV, dtype=dtype)
    t = np.linspace(0., 2., 4)
    sol, st = rows_call(PC.time_callable, y0, t)
    assert st['lower']['lowered'] is True and st['lower']['kind'] == 'rowlocal', st['lower']
    assert int(st['rows']['n_attempts'].min()) < int(st['rows']['n_attempts'].max())
    for i in (0, 33, 69):
        ref = odeint(PC.time_callable, y0[i:i + 1], torch.as_tensor(t), method='dopri5', options={'lower': True}, **TOL[dtype])
        rs = dict(odeint.last_stats)
        assert rs['lower']['lowered'] is True and rs['n_launches'] == 1
        assert torch.equal(sol[:, i], ref[:, 0])
        assert (int(st['rows']['n_attempts'][i]), int(st['rows']['n_accepted'][i])) == (rs['n_attempts'], rs['n_accepted'])
    if dtype == F64:
        ref, counts = oracle_rows(('time', dtype), PC.time_np, y0.cpu().numpy(), t, 'dopri5', TOL[F64])
        assert list(zip(st['rows']['n_attempts'].cpu().tolist(), st['rows']['n_accepted'].cpu().tolist())) == counts
        band64(sol.cpu().numpy(), ref, 'lowered callable')


# ---- a failing row: a numerical status, never a fault ----------------------------------------------------------------------------------------------------
def test_a_row_that_blows_up_fails_alone():
    f = PC.blow_up()
    y0 = torch.tensor([[0.1], [1.0], [0.2]], dtype=F64, device=DEV)
    with pytest.raises(AssertionError) as e:
        odeint(f, y0, torch.tensor([0., 2.]), method='dopri5', options={'per_trajectory': True}, **TOL[F64])
    msg = str(e.value)
    assert 'underflow in dt' in msg and '1 of 3 rows failed' in msg and 'rows 1,' in msg and "row 1's" in msg, msg
    with pytest.raises(AssertionError) as e1:               # the message is the batch-1 call's, with the row's own dt
        odeint(f, y0[1:2], torch.tensor([0., 2.]), method='dopri5', **TOL[F64])
    assert msg.startswith(str(e1.value) + ' [per_trajectory'), (msg, str(e1.value))
    # the healthy rows were integrated to the end: y(2) = y0 / (1 - 2 y0)
    sol = odeint(f, y0[[0, 2]].contiguous(), torch.tensor([0., 2.]), method='dopri5', options={'per_trajectory': True}, **TOL[F64])
    assert torch.allclose(sol[1, :, 0], torch.tensor([0.1 / 0.8, 0.2 / 0.6], dtype=F64, device=DEV), rtol=1e-5, atol=0)


def test_max_num_steps_raises_the_reference_message():
    y0 = base(F64)
    with pytest.raises(AssertionError) as e:
        odeint(rhs.Lorenz(), y0, torch.as_tensor(PC.BASE_T), method='dopri5', options={'per_trajectory': True, 'max_num_steps': 3}, **TOL[F64])
    assert str(e.value).startswith('max_num_steps exceeded (3>=3)') and '70 of 70 rows failed' in str(e.value), str(e.value)


def test_c_abi_refuses_a_handle_that_is_not_trajectory_per_thread():
    from tfdiffeq_amd.dopri5 import _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID
    from tfdiffeq_amd.solvers import _FusedEngine
    W = torch.eye(16, dtype=F64, device=DEV) * -0.5
    eng = _FusedEngine(rhs.Linear(W), torch.ones(8, 16, dtype=F64, device=DEV), True, _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID)
    try:
        with pytest.raises(N.NativeError) as e:
            eng.integrate_rows(np.array([0., 1.]))
        assert e.value.rc == N.E_INVALID and 'not trajectory-per-thread' in str(e.value)
    finally:
        eng.close()


def test_reruns_are_bit_identical():
    y0 = base(F64)
    a, sa = rows_call(rhs.Lorenz(), y0, PC.BASE_T)
    b, sb = rows_call(rhs.Lorenz(), y0, PC.BASE_T)
    assert torch.equal(a, b) and all(torch.equal(sa['rows'][k], sb['rows'][k]) for k in sa['rows'])
