"""GPU tests of the one-launch hypersolver kernels (csrc/mi_ode_hyper.h) at their edges, against the numpy restatement of the reference's
hypersolvers (tests/hyper_restatement.py): time-dependent systems on non-uniform grids (the stage times and dt = t[1] - t[0]), every
catalogue system, state widths 1 .. 32, 2 .. 6 layers, hidden widths 1 .. 128, every activation and bias layout, both sides of the LDS
budget in both dtypes, the grid-stride trips of all three kernels, row independence and isolation by torch.equal, one solver object reused.
Cases, inputs and bounds: tests/hyper_cases.py (checked on the CPU by tests/test_hyper_cases_host.py); nothing measured here enters a bound.
Run with -s for every deviation next to its bound."""
import numpy as np
import pytest
import torch

from tests import bands
from tests import hyper_cases as C
from tests import hyper_restatement as HR
from tfdiffeq_amd import hyper_solvers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SOLVERS = {'euler': H.HyperEuler, 'midpoint': H.HyperMidpoint, 'heun': H.HyperHeun, 'resid': H.HyperEuler, 'gresid': H.HyperEuler}
WORST = {}                      # (dtype, path) -> (share of the bound, deviation, bound, case, op)


def dev(case, a):
    return torch.tensor(np.asarray(a), dtype=getattr(torch, case.dtype), device=DEV)


def solver_of(case, op):
    f, opts = C.make_f(case)
    return SOLVERS[op](f, C.make_g(case, DEV), options=opts)


def call(s, case, op, t, y):
    """One call of `op` on the state / base trajectory y; asserts the fused engine and its launch count."""
    if op in C.TRAJ_OPS:
        out = s.trajectory(t, y)
    elif op == 'resid':
        out = s.residual_trajectory(t, y)
    else:
        out = s._hypersolver_residuals(t, y)
    assert s.last_stats['engine'] == 'fused', s.last_stats
    assert s.last_stats['n_launches'] == C.launches_of(case, op), s.last_stats
    return out


def state_of(case, op, rows=None):
    y = C.y0_of(case) if op in C.TRAJ_OPS else C.base_of(case)
    if rows is not None:
        y = y[rows] if op in C.TRAJ_OPS else y[:, rows]
    return dev(case, y)


def run(case, op, rows=None, s=None):
    s = solver_of(case, op) if s is None else s
    return call(s, case, op, dev(case, C.grid_of(case)), state_of(case, op, rows))


@pytest.mark.parametrize('case,op', C.pairs(), ids=['%s-%s' % (c.name, op) for c, op in C.pairs()])
def test_parity_with_the_restatement(case, op):
    out = run(case, op)
    ref = C.reference(case, op)
    assert out.dtype == getattr(torch, case.dtype) and tuple(out.shape) == ref.shape
    obs, bound = bands.observed(out.cpu().numpy(), ref), C.bound_of(case, op)
    key = (case.dtype, C.path_of(case) if op != 'resid' else 'no net')
    if key not in WORST or obs / bound > WORST[key][0]:
        WORST[key] = (obs / bound, obs, bound, case.name, op)
    print('%s %s [%s, %s]: max |got - ref| / (1 + |ref|) = %.3e, bound %.3e' % (case.name, op, case.dtype, key[1], obs, bound))
    assert obs <= bound


def test_the_exact_budget_net_launches_with_the_whole_lds():
    """5-128-96-2 in float64: 163 840 bytes of dynamic LDS, all a compute unit has.  It must launch (one launch: the weights in LDS) and
    be right in the trajectory kernel and in the MODE 2 residual kernel."""
    case = C.BY_NAME['lds_exact']
    assert C.lds_bytes(case) == 160 * 1024
    for op in ('heun', 'gresid'):
        s = solver_of(case, op)
        out = run(case, op, s=s)
        assert s.last_stats['n_launches'] == 1
        assert bands.observed(out.cpu().numpy(), C.reference(case, op)) <= C.F64_BOUND


@pytest.mark.parametrize('op', C.ALL_OPS)
@pytest.mark.parametrize('name', ['w50_prelu1', 'ring17', 'l2_over', 'f32_l4_mixed'])
def test_rows_do_not_depend_on_their_tile(name, op):
    """Rows 0, 15, 16 and 36 of a 37-row call equal the same rows run alone: the k-order of the chains does not depend on the row."""
    case = C.BY_NAME[name]
    s = solver_of(case, op)
    whole = run(case, op, s=s)
    for r in (0, 15, 16, 36):
        alone = run(case, op, rows=slice(r, r + 1), s=s)
        assert torch.equal(alone[:, 0], whole[:, r]), (name, op, r)


@pytest.mark.parametrize('op', C.TRAJ_OPS)
def test_the_single_row_of_the_second_trip_equals_its_own_run(op):
    case = C.BY_NAME['trip2']
    r = C.ROWS * C.MAX_GRID
    assert case.B == r + 1
    s = solver_of(case, op)
    whole = run(case, op, s=s)
    alone = run(case, op, rows=slice(r, r + 1), s=s)
    assert torch.equal(alone[:, 0], whole[:, r])
    first = run(case, op, rows=slice(0, 1), s=s)                 # (and the first row of the first trip of the same workgroup)
    assert torch.equal(first[:, 0], whole[:, 0])


@pytest.mark.parametrize('op', C.ALL_OPS)
@pytest.mark.parametrize('name', ['w15_relu_b15', 'w50_prelu1', 'f32_w127_softplus'])
def test_non_finite_rows_stay_in_their_rows(name, op):
    """A NaN row and an inf row in the ragged last tile (and a NaN row in a full one): every other row is bit for bit the run without them,
    and a clean call afterwards is correct."""
    case = C.BY_NAME[name]
    s = solver_of(case, op)
    t = dev(case, C.grid_of(case))
    clean_in = state_of(case, op)
    clean = call(s, case, op, t, clean_in).clone()
    bad_rows = [r for r in (5, case.B - 4, case.B - 2) if 0 <= r < case.B]
    dirty_in = clean_in.clone()
    for j, r in enumerate(bad_rows):
        dirty_in[..., r, :] = float('inf') if j == 2 else float('nan')
    dirty = call(s, case, op, t, dirty_in)
    keep = [r for r in range(case.B) if r not in bad_rows]
    assert torch.equal(dirty[:, keep], clean[:, keep])
    assert bool(torch.isnan(dirty[-1, bad_rows[:2]]).all())       # (the NaN rows stay NaN; what inf becomes depends on the net)
    again = call(s, case, op, t, clean_in)
    assert torch.equal(again, clean)
    assert bands.observed(again.cpu().numpy(), C.reference(case, op)) <= C.bound_of(case, op)


def test_one_solver_object_through_batches_grids_and_dtypes():
    """Another batch size, another grid and a float32 copy of g through the same object, then the first call again bit for bit."""
    case = C.BY_NAME['w50_prelu1']
    s = solver_of(case, 'heun')
    g64 = s.g
    t, y0 = dev(case, C.grid_of(case)), dev(case, C.y0_of(case))
    first = call(s, case, 'heun', t, y0).clone()
    five = call(s, case, 'heun', t, y0[:5])
    assert torch.equal(five, first[:, :5])
    td = dev(case, C.DECREASING)
    back = call(s, case, 'heun', td, y0)
    ref = HR.trajectory('heun', C.f_np(case), C.layers_of(case), C.DECREASING, C.y0_of(case))
    assert bands.observed(back.cpu().numpy(), ref) <= C.F64_BOUND
    c32 = C.BY_NAME['f32_w50_prelu1_tanh']
    s.g = C.make_g(c32, DEV)
    out32 = call(s, c32, 'heun', dev(c32, C.grid_of(c32)), dev(c32, C.y0_of(c32)))
    assert out32.dtype == torch.float32
    assert bands.observed(out32.cpu().numpy(), C.reference(c32, 'heun')) <= C.bound_of(c32, 'heun')
    big = C.BY_NAME['l2_over']                                   # ... and a net that goes through the workspace
    s.g = C.make_g(big, DEV)
    outb = call(s, big, 'heun', t, y0)
    assert bands.observed(outb.cpu().numpy(), C.reference(big, 'heun')) <= C.F64_BOUND
    s.g = g64
    assert torch.equal(call(s, case, 'heun', t, y0), first)
    assert bands.observed(first.cpu().numpy(), C.reference(case, 'heun')) <= C.F64_BOUND


def test_zz_worst_deviation_per_dtype_and_path():
    """The log's summary (python -m pytest -s): the worst share of its bound per dtype and weight path among the parity cases run before."""
    for (dtype, path), (share, obs, bound, name, op) in sorted(WORST.items()):
        print('worst %s / %s: %.3e of bound %.3e (%.1f %%) at %s %s' % (dtype, path, obs, bound, 100 * share, name, op))
        assert share <= 1.0
