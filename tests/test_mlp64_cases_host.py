"""CPU checks of the inputs of tests/test_gpu_mlp64_edges.py (tests/mlp64_cases.py): the oracle is run once per adaptive case and must show
what the GPU tests rely on - a clean finite solution, rejected attempts where the case is marked rejecting, every attempt's error ratio
farther than 1e-9 from 1.0 (a summation-order difference on the device then cannot fork the accept / reject sequence), several output times
inside one accepted step for the dense-output cases - so that a GPU failure cannot be blamed on the inputs."""
import numpy as np
import pytest

from tests import mlp64_cases as MC


@pytest.mark.parametrize('case', MC.ADAPTIVE_CASES, ids=MC.ids(MC.ADAPTIVE_CASES))
def test_adaptive_case_is_clean_decided_and_rejecting_where_marked(case):
    ref, st, ratios = MC.oracle(case)                       # (an oracle assertion - dt underflow, non-finite state - fails the test here)
    assert ref.shape == (len(case.t), MC.batch_of(case), case.d) and np.isfinite(ref).all()
    assert len(ratios) == st.n_attempts >= 2
    gap = float(np.min(np.abs(np.array(ratios) - 1.0)))
    assert gap > 1e-9, (gap, ratios)
    assert [r <= 1.0 for r in ratios] == [bool(row[2]) for row in st.trace]
    if case.rejecting:
        assert st.n_attempts - st.n_accepted >= 1, ratios
    # the kernels hold 1e-9 ABSOLUTE: the solution must stay of order one for that to be a float64 statement
    assert float(np.abs(ref).max()) < 50.0


def test_handle_case_is_decided_at_the_large_batch_too():
    ref, st, ratios = MC.oracle(MC.HANDLE, batch=MC.B2())
    assert np.isfinite(ref).all() and float(np.min(np.abs(np.array(ratios) - 1.0))) > 1e-9


@pytest.mark.parametrize('case', MC.MULTI_FIXED + MC.FIXED_OPTIONS, ids=MC.ids(MC.MULTI_FIXED + MC.FIXED_OPTIONS))
def test_fixed_grid_case_is_finite_and_of_order_one(case):
    ref, _, _ = MC.oracle(case)
    assert ref.shape == (len(case.t), MC.batch_of(case), case.d) and np.isfinite(ref).all() and float(np.abs(ref).max()) < 50.0
    if case.options and case.options[0][0] == 'step_size':   # the requested times lie strictly between the points of the solver's own grid
        grid = np.arange(8) * case.options[0][1]
        assert all(np.min(np.abs(grid - x)) > 1e-3 for x in case.t[1:-1])


@pytest.mark.parametrize('case', MC.DENSE, ids=MC.ids(MC.DENSE))
def test_dense_case_has_a_step_with_several_outputs(case):
    _, st, _ = MC.oracle(case)
    per_step = MC.steps_with_outputs(case, st)
    assert sum(per_step) == len(case.t) - 1
    assert max(per_step) >= 3, per_step
    t = np.array(case.t)
    assert len(t) == 40 and np.all(np.diff(t) > 0) and float(np.min(np.diff(t))) <= 1e-12 + 1e-16


def test_every_case_family_covers_what_it_is_for():
    geoms = lambda cases: {MC.geometry(c.d, c.h) for c in cases}   # noqa: E731
    both = {(16, 16), (64, 128)}
    for fam in (MC.MULTI_ADAPTIVE, MC.MULTI_FIXED, MC.SCHEDULES, MC.DENSE, MC.FIXED_OPTIONS):
        assert geoms(fam) == both
    for g in both:
        fam = [c for c in MC.MULTI_ADAPTIVE if MC.geometry(c.d, c.h) == g]
        assert {c.method for c in fam} == {'dopri5', 'tsit5', 'bosh3', 'dopri8'}
        assert any(c.td for c in fam) and any(c.t[0] > c.t[-1] for c in fam) and all(c.rejecting for c in fam)
        assert [c.batch for c in fam if c.method != 'dopri5'] == ['B2'] * 3 and {c.batch for c in fam if c.method == 'dopri5'} == {'B2', 'B3'}
    assert {c.method for c in MC.SCHEDULES} == {'dopri5', 'tsit5', 'bosh3', 'dopri8'}
    assert any(c.td for c in MC.SCHEDULES) and any(c.t[0] > c.t[-1] for c in MC.SCHEDULES) and any(c.batch == 'B2' for c in MC.SCHEDULES)
    assert sum(c.first_step is not None for c in MC.SCHEDULES) == 2
    assert any(g[0] > g[-1] and len(set(np.round(np.diff(g), 12))) > 1 for g in (c.t for c in MC.MULTI_FIXED))
    assert all(len(c.t) == 4 for c in MC.MULTI_FIXED)
    assert [(c.d, c.h) for c in MC.WIDTH_EDGES] == MC.WIDTHS and all(MC.batch_of(c) == 65 for c in MC.WIDTH_EDGES)
    assert {c.act for c in MC.WIDTH_EDGES} == {'tanh', 'relu', 'softplus'} and sum(not c.bias for c in MC.WIDTH_EDGES) == 2
    assert {c.td for c in MC.WIDTH_EDGES} == {False, True}
    assert MC.geometry(16, 17) == MC.geometry(17, 16) == (64, 128) and MC.geometry(16, 16) == MC.geometry(1, 1) == (16, 16)


@pytest.mark.parametrize('cus', [1, 8, 104, 120, 228, 256, 304])
def test_device_dependent_batches_put_a_one_row_tile_on_a_later_trip(cus):
    for B, trips in ((MC.B2(cus), 2), (MC.B3(cus), 3)):
        assert MC.n_tiles(B) > cus and B % MC.TILE == 1
        assert -(-MC.n_tiles(B) // cus) >= trips and (MC.n_tiles(B) - 1) // cus >= 1      # the ragged tile is not on a first trip
    # B2: workgroups 0 and 1 make two trips, the others one - unequal trip counts in front of the grid-wide reduction
    assert MC.n_tiles(MC.B2(cus)) == cus + 2


def test_status_case_needs_more_than_three_attempts_in_one_interval():
    from oracle import ode_numpy as O
    _, f, y0, t = MC.inputs(MC.STATUS)
    with pytest.raises(AssertionError, match='max_num_steps exceeded'):
        O.odeint(f, y0, t, rtol=MC.STATUS.rtol, atol=MC.STATUS.atol, method='dopri5', options={'max_num_steps': 3})
    y0[-1, 3] = np.nan
    # dopri5.py:99-100.  (With the automatic first step the reference never gets there: the step size is NaN and the assertion one line
    # above, :98, fires first - 'underflow in dt nan'.  The fused kernels raise the flag in their first pass over y0 and report the state.)
    with pytest.raises(AssertionError, match='non-finite'):
        O.odeint(f, y0, t, rtol=MC.STATUS.rtol, atol=MC.STATUS.atol, method='dopri5', options={'first_step': 0.01})
    with pytest.raises(AssertionError, match='underflow in dt nan'):
        O.odeint(f, y0, t, rtol=MC.STATUS.rtol, atol=MC.STATUS.atol, method='dopri5')


@pytest.mark.parametrize('d,h', [MC.G64, MC.G16])
def test_saturated_inputs_reach_every_arm_of_the_activations(d, h):
    ws, y0 = MC.saturated(d, h)
    assert float(np.abs(y0).max()) <= 1.0
    z = y0 @ ws[0] + ws[1]                                  # layer-1 pre-activations
    z0 = z[0]
    for v in (0.0625, 30.0):
        for lo, hi in ((v * (1 - 2e-3), v), (v, v * (1 + 2e-3))):
            assert np.any((z0 > lo) & (z0 < hi)) and np.any((-z0 > lo) & (-z0 < hi)), (v, lo, hi)
    assert z.max() > 710.0 and z.min() < -710.0
    for act in ('tanh', 'relu', 'softplus'):
        out = y0 + MC.np_f(ws, act, False)(0.0, y0)
        assert np.isfinite(out).all()


def test_numpy_restatement_against_torch():
    import torch
    for case in (MC.WIDTH_EDGES[1], MC.WIDTH_EDGES[2], MC.WIDTH_EDGES[3], MC.WIDTH_EDGES[9]):
        ws, f, y0, _ = MC.inputs(case)
        m = MC.to_mlp(ws, case.act, case.td, 'cpu')
        got = m.forward(0.3, torch.tensor(y0)).numpy()
        assert float(np.abs(got - f(0.3, y0)).max()) < 1e-12


@pytest.mark.parametrize('d,h', [(16, 17), (17, 16), (6, 16)])
def test_plan_names_the_float64_tile_kernel(d, h):
    """What the width-edge GPU tests assert of odeint.plan, here without a device: the float64 tile kernel, not the cooperative one."""
    import torch
    from tfdiffeq_amd import odeint
    ws = MC.make_net(d, h, 5)
    p = odeint.plan(MC.to_mlp(ws, 'tanh', False, 'cpu'), torch.zeros(65, d, dtype=torch.float64), torch.tensor([0., 1.]), method='dopri5')
    assert p['engine'] == 'fused' and p['kernel'].startswith('k_persist_mlp64<') and 'Coop' not in p['kernel'], p
