"""Per-trajectory step control for the ODEFunc network on the GPU (options={'per_trajectory': True} with an rhs.MLP; csrc/mi_ode_rows_mlp.h,
k_rows_mlp): a 32-row tile per workgroup, workgroup-uniform control flow, every row its own step, record, controller and output cursor.

What is held, and to what (cases: tests/per_trajectory_mlp_cases.py - every tile geometry, batches 1 / 31 / 32 / 33 / 70, three tableaus, three
activations, with and without the time input, forward and reversed t, T = 1 / 2 / 5 / 40, the grid clamped to 1 and 2 workgroups):
  * invariance, bitwise (torch.equal, per-row counts included): the batch against the same rows in another order (other tile positions,
    other tile-mates), against y0[i:i+1] with the option on, and against a second run;
  * the batch-of-one call WITHOUT the option on the existing float32 MLP engine: attempts and accepted counts equal, values within
    bands.case_ceiling(attempts of that row, stages = S + 1) - the arithmetic is the same, the order of a row's norm reduction follows the
    shared kernels' one-row block reduction (csrc/mi_ode_rows_mlp.h), so bit equality is the aim and is printed per case;
  * the float64 oracle (oracle/ode_numpy.py) on each sampled row alone: values within the same ceiling from the ORACLE's attempt count of
    that row; the oracle's counts over the rows take more than one value (divergent control is exercised).  The ceiling takes growth = 1,
    so these cases are nets whose flow provably does not expand, at a tolerance below the ceiling (per_trajectory_mlp_cases.ORACLE says
    why; a first version held the dense random nets to it: row 31 of ragged_tanh_b70_dopri5_tdep_grid1, bit-equal to the shared kernel,
    was 2.5e-4 from the oracle against 2.7e-5 - that net amplifies a perturbation 60 times).  method='tsit5' is the published tableau:
    the oracle's options['tsit5_fixed'], as in tests/test_gpu_parity.py;
  * failing rows are status exits (a NaN in y0, max_num_steps, the only row of a second tile): the row carries its bit, the others are
    the rows of the batch without it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_trajectory_mlp_cases as MC                      # noqa: E402
from tests.bands import case_ceiling, observed            # noqa: E402
from tfdiffeq_amd import _native as N                     # noqa: E402
from tfdiffeq_amd import odeint, rhs                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ENGINE = 'k_rows_mlp: per-trajectory step control on the MLP tile kernel: a 32-row tile per workgroup, every row its own control, one launch'
KEYS = ('n_attempts', 'n_accepted', 'nfe', 'status')

_FUNC, _FULL = {}, {}


def func_of(case):
    if case.name not in _FUNC:
        W1, b1, W2, b2, W3, b3 = [torch.tensor(a, device=DEV) for a in MC.weights(case)]
        _FUNC[case.name] = rhs.MLP(W1, b1, W2, b2, W3, b3, activation=case.act, time_dependent=case.tdep)
    return _FUNC[case.name]


def y0_of(case):
    return torch.tensor(MC.y0(case), device=DEV)


def rows_call(case, y0, **extra):
    sol = odeint(func_of(case), y0, torch.tensor(case.t, dtype=torch.float64), method=case.method,
                 options=dict(case.opts, per_trajectory=True, **extra), **MC.tol(case))
    st = dict(odeint.last_stats)
    assert st['engine'] == ENGINE and st['kernel'] == 'k_rows_mlp' and st['n_launches'] == 1 and st['per_trajectory'] is True, st
    assert st['status'] == 0 and st['route'] == 'fused_rows_mlp', st
    return sol, st


def full(case):
    """The full-batch result of a case, computed once and shared (never modified)."""
    if case.name not in _FULL:
        _FULL[case.name] = rows_call(case, y0_of(case))
    return _FULL[case.name]


def counts(st, i):
    return tuple(int(st['rows'][k][i]) for k in KEYS)


# ---- 1, 2, 6: the edge grid, invariance and the stats ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c.name for c in MC.CASES])
def test_rows_do_not_depend_on_their_batch(name):
    case = MC.BY_NAME[name]
    y0 = y0_of(case)
    sol, st = full(case)
    B, T = case.batch, len(case.t)
    assert sol.shape == (T, B, case.dim) and sol.dtype == torch.float32 and torch.equal(sol[0], y0)
    assert bool(torch.isfinite(sol).all())
    r = st['rows']
    assert sorted(r) == sorted(KEYS) and all(r[k].shape == (B,) and r[k].dtype == torch.int64 and r[k].is_cuda for k in KEYS)
    assert (st['n_attempts'], st['n_accepted'], st['nfe']) == (int(r['n_attempts'].max()), int(r['n_accepted'].max()), int(r['nfe'].max()))
    assert int(r['status'].max()) == 0
    if T > 1 and B > 1:
        assert len(set(r['n_attempts'].tolist())) > 1, 'the rows of this case should need different numbers of attempts'
    # a second run of the same call
    sol2, st2 = rows_call(case, y0)
    assert torch.equal(sol2, sol) and all(torch.equal(st2['rows'][k], r[k]) for k in KEYS)
    # the same rows in another order: other tile positions, other tile-mates
    p = torch.tensor(MC.perm(B), device=DEV)
    solp, stp = rows_call(case, y0[p].contiguous())
    back = torch.empty_like(solp)
    back[:, p] = solp
    assert torch.equal(back, sol), float((back - sol).abs().max())
    for k in KEYS:
        bk = torch.empty_like(stp['rows'][k])
        bk[p] = stp['rows'][k]
        assert torch.equal(bk, r[k]), k
    # every sampled row alone, with the option on
    for i in MC.sample_rows(B):
        sol1, st1 = rows_call(case, y0[i:i + 1].contiguous())
        assert torch.equal(sol1[:, 0], sol[:, i]), (i, float((sol1[:, 0] - sol[:, i]).abs().max()))
        assert counts(st1, 0) == counts(st, i), (i, counts(st1, 0), counts(st, i))


def test_the_grid_clamp_changes_no_bit():
    """Batch 70 is 3 tiles: one workgroup walks all three, two workgroups walk two and one, three take one each."""
    case = MC.BY_NAME['ragged_tanh_b70_dopri5_tdep_grid1']
    sol, st = full(case)                                      # (the case itself runs with the grid clamped to 1)
    for g in (0, 2, 3):
        solg, stg = rows_call(case, y0_of(case), rows_grid=g)
        assert torch.equal(solg, sol) and all(torch.equal(stg['rows'][k], st['rows'][k]) for k in KEYS), g


# ---- 3: the batch-of-one call on the existing shared-control engine ------------------------------------------------------------------------
@pytest.mark.parametrize('name', MC.SHARED_CASES)
def test_rows_against_shared_control_on_one_row(name):
    case = MC.BY_NAME[name]
    y0 = y0_of(case)
    sol, st = full(case)
    S, equal, worst = MC.STAGES[case.method], 0, 0.0
    rows = MC.sample_rows(case.batch)
    for i in rows:
        ref = odeint(func_of(case), y0[i:i + 1].contiguous(), torch.tensor(case.t, dtype=torch.float64), method=case.method, **MC.TOL)
        rs = dict(odeint.last_stats)
        assert rs.get('per_trajectory') is None, rs
        got = counts(st, i)
        obs = observed(sol[:, i].cpu().numpy(), ref[:, 0].cpu().numpy())
        equal += int(torch.equal(sol[:, i], ref[:, 0]))
        worst = max(worst, obs)
        print('%s row %d: attempts %d (shared %d), accepted %d (shared %d), observed %.3e, ceiling %.3e, bit-equal %s'
              % (name, i, got[0], rs['n_attempts'], got[1], rs['n_accepted'], obs, case_ceiling(got[0], stages=S + 1), torch.equal(sol[:, i], ref[:, 0])))
        assert (got[0], got[1]) == (rs['n_attempts'], rs['n_accepted']), (i, got, rs['n_attempts'], rs['n_accepted'])
        assert obs <= case_ceiling(got[0], stages=S + 1), (i, obs, case_ceiling(got[0], stages=S + 1))
    print('%s: %d of %d sampled rows bit-equal to the batch-of-one call, largest difference %.3e' % (name, equal, len(rows), worst))


# ---- 4: the float64 oracle on every sampled row alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MC.ORACLE_CASES)
def test_rows_against_the_float64_oracle(name):
    case = MC.BY_NAME[name]
    sol, st = full(case)
    rows = MC.sample_rows(case.batch)
    refs, cnt = MC.oracle_rows(case, rows)
    assert len({cnt[i][0] for i in rows}) > 1, 'the oracle should need different numbers of attempts for these rows: %s' % cnt
    S = MC.STAGES[case.method]
    got = sol.cpu().numpy()
    for i in rows:
        obs, ceil = observed(got[:, i], refs[i]), case_ceiling(cnt[i][0], stages=S + 1)
        print('%s row %d: attempts %d (oracle %d), observed %.3e, ceiling %.3e' % (name, i, counts(st, i)[0], cnt[i][0], obs, ceil))
    for i in rows:
        obs, ceil = observed(got[:, i], refs[i]), case_ceiling(cnt[i][0], stages=S + 1)
        assert obs <= ceil, (name, i, obs, ceil)


# ---- 5: failing rows (status exits) ----------------------------------------------------------------------------------------------------------
def engine_rows(case, y0, **opts):
    """The C entry point below the solver: (solution, [batch, 4] rows, OR of the status bits) - nothing raises on a failing row."""
    from tfdiffeq_amd.misc import _TupleFunc
    from tfdiffeq_amd.odeint import SOLVERS
    s = SOLVERS[case.method](_TupleFunc(func_of(case)), (y0,), per_trajectory=True, **MC.TOL, **opts)
    route = s.route()
    assert route.kind == 'fused_rows_mlp'
    return s._make_engine(route).integrate_rows_mlp(np.asarray(case.t, dtype=np.float64), y0, 0)


def test_a_nan_row_fails_alone():
    case = MC.BY_NAME['g16x16_tanh_b70_dopri5']
    y0 = y0_of(case)
    bad = 17
    y0n = y0.clone()
    y0n[bad, 1] = float('nan')
    out, rows, bits = engine_rows(case, y0n)
    assert bits == N.ST_NONFINITE and int(rows[bad, 3]) == N.ST_NONFINITE and int(rows[bad, 0]) == 0
    keep = [i for i in range(case.batch) if i != bad]
    assert int(rows[keep, 3].max()) == 0
    ref, ref_rows, ref_bits = engine_rows(case, y0[keep].contiguous())
    assert ref_bits == 0 and torch.equal(out[:, keep], ref) and torch.equal(rows[keep], ref_rows)
    with pytest.raises(AssertionError) as e:
        odeint(func_of(case), y0n, torch.tensor(case.t, dtype=torch.float64), method=case.method, options={'per_trajectory': True}, **MC.TOL)
    assert 'per_trajectory: 1 of 70 rows failed; rows 17,' in str(e.value), str(e.value)


def test_max_num_steps_stops_the_slow_rows_only():
    case = MC.BY_NAME['g16x16_softplus_b31_bosh3']            # one output interval: a row fails iff it needs more than the limit
    y0 = y0_of(case)
    sol, st = full(case)
    att = st['rows']['n_attempts']
    limit = int(att.median())
    slow = (att > limit).nonzero().flatten().tolist()
    fast = (att <= limit).nonzero().flatten().tolist()
    assert slow and fast, att.tolist()
    out, rows, bits = engine_rows(case, y0, max_num_steps=limit)
    assert bits == N.ST_MAX_STEPS
    assert rows[slow, 3].tolist() == [N.ST_MAX_STEPS] * len(slow) and rows[slow, 0].tolist() == [limit] * len(slow)
    assert int(rows[fast, 3].max()) == 0 and torch.equal(out[:, fast], sol[:, fast]) and torch.equal(rows[fast, 0], att[fast])
    with pytest.raises(AssertionError) as e:
        odeint(func_of(case), y0, torch.tensor(case.t, dtype=torch.float64), method=case.method,
               options={'per_trajectory': True, 'max_num_steps': limit}, **MC.TOL)
    msg = str(e.value)
    assert msg.startswith('max_num_steps exceeded (%d>=%d)' % (limit, limit)), msg
    assert 'per_trajectory: %d of %d rows failed; rows %s' % (len(slow), case.batch, ', '.join(str(i) for i in slow[:8])) in msg, msg


def test_the_only_row_of_a_second_tile_fails_alone():
    case = MC.BY_NAME['g16x16_relu_b33_tsit5_tdep']           # batch 33: row 32 is the second tile
    y0 = y0_of(case)
    sol, st = full(case)
    y0n = y0.clone()
    y0n[32, 0] = float('inf')
    out, rows, bits = engine_rows(case, y0n)
    assert bits == N.ST_NONFINITE and int(rows[32, 3]) == N.ST_NONFINITE
    assert int(rows[:32, 3].max()) == 0 and torch.equal(out[:, :32], sol[:, :32])
    assert all(torch.equal(rows[:32, j], st['rows'][k][:32]) for j, k in enumerate(KEYS))


# ---- the C ABI and the public surface ----------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_a_handle_outside_the_box():
    from tfdiffeq_amd.dopri5 import _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID
    from tfdiffeq_amd.solvers import _FusedEngine
    eng = _FusedEngine(rhs.Lorenz(), torch.ones(8, 3, dtype=torch.float32, device=DEV), True, _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID)
    try:
        with pytest.raises(N.NativeError) as e:
            eng.integrate_rows_mlp(np.array([0., 1.]))
        assert e.value.rc == N.E_INVALID and 'ODEFunc network' in str(e.value)
    finally:
        eng.close()


def test_odeblock_inference_reaches_the_route():
    from tfdiffeq_amd import models
    torch.manual_seed(0)
    block = models.ODEBlock(models.ODEFunc(6, 16, non_linearity='tanh'), tol=1e-4).to(DEV)
    block.options = {'per_trajectory': True}
    x = torch.randn(40, 6, generator=torch.Generator().manual_seed(1)).to(DEV) * torch.logspace(-1, 1, 40, device=DEV)[:, None]
    with torch.no_grad():
        out = block(x)
    st = dict(odeint.last_stats)
    assert st['kernel'] == 'k_rows_mlp' and st['n_launches'] == 1 and out.shape == (40, 6), st
    with torch.no_grad():
        one = block(x[7:8])
    assert torch.equal(one[0], out[7])
