"""CPU checks of tests/hyper_cases.py: every case of the hypersolver edge suite (tests/test_gpu_hyper_edges.py) can show the defects it is
there for - in the float64 restatement each wrong variant differs from the right result by more than 100 x the case's bound - the activation
cases reach both branches, every net is on the side of the LDS budget its name says, the float32 bounds are what the issue's scheme gives and
stay below 1e-4, and the float32 restatement agrees with torch's own float32 eager loop.  No GPU needed."""
import numpy as np
import pytest
import torch

from tests import bands
from tests import hyper_cases as C
from tests import hyper_restatement as HR
from tfdiffeq_amd import _native as N
from tfdiffeq_amd import hyper_solvers as H

SMALL = [c for c in C.CASES if c.B <= 64]
F64 = [c for c in C.CASES if c.dtype == 'float64']
F32 = [c for c in C.CASES if c.dtype == 'float32']


def test_hyper_sources_are_hyper_translation_units():
    src = C.hyper_sources()
    assert len(src) >= 9                                        # forced x 2 dtypes, the lowered callable, ring at 6 widths (+ 2 in float32)
    assert all('MI_ODE_DEFINE_HYPER_PLUGIN' in s and '#include "mi_ode_hyper_plugin.h"' in s for s in src)
    assert len(set(src)) == len(src)
    for D in (1, 7, 8, 16, 17, 32):
        assert any(C.ring_body(D) in s for s in src)


def test_the_cases_cover_what_the_issue_lists():
    layer_counts = set(len(c.hidden) + 1 for c in F64)
    assert layer_counts == {2, 3, 4, 5, 6}
    assert {1, 15, 16, 17, 50, 112, 127, 128} <= set(h for c in F64 for h in c.hidden)
    for dtype_cases in (F64, F32):
        acts = set(a for c in dtype_cases for a in c.acts[:-1])
        assert acts == {'relu', 'leaky', 'prelu', 'prelu1', 'tanh', 'softplus', None}
        assert any(c.acts[-1] == 'tanh' for c in dtype_cases)
        assert any(not all(c.bias) for c in dtype_cases)
        assert any(c.first_scale > 1 and 'softplus' in c.acts for c in dtype_cases)
    assert any(c.identity for c in F64)
    assert any(not c.bias[-1] for c in F64) and any(not all(c.bias[1:-1]) for c in F64 if len(c.bias) > 2)
    assert {1, 15, 16, 17, 37} <= set(c.B for c in F64)
    assert set(c.system for c in F64) == set(C.SYSTEMS)
    assert set(c.D for c in F64 if c.system == 'ring') == {1, 7, 8, 16, 17, 32}
    assert set(c.D for c in F32 if c.system == 'ring') == {8, 32}
    assert {'main', 'decreasing', 'two'} <= set(c.grid for c in F64)
    for c in F64:
        if c.B <= 64:
            assert set(c.ops) == set(C.ALL_OPS)
    # the trips: a second trip of workgroup 0 with ONE live row, a third trip, MODE 2 over 32768 rows with two time indices in one tile,
    # MODE 1 over 2048 * 256 rows
    assert C.BY_NAME['trip2'].B == 16 * 2048 + 1 and C.BY_NAME['trip3'].B == 16 * 4096 + 5
    g = C.BY_NAME['trip_gresid']
    assert 3 * g.B > 16 * 2048 and g.B % 16 != 0 and len(C.GRIDS[g.grid]) == 3
    r = C.BY_NAME['trip_resid']
    assert (len(C.GRIDS[r.grid]) - 1) * r.B > 2048 * 256
    assert C.path_of(C.BY_NAME['trip_gresid_l2']) == 'l2'


def test_grids_step_by_t1_minus_t0_and_are_not_uniform():
    for name in ('main', 'decreasing', 'fine'):
        g = np.asarray(C.GRIDS[name])
        assert not C.uniform(C.Case('x', 'forced', [1], ['tanh'], grid=name))
        dt = g[1] - g[0]
        off = np.abs((g - (g[0] + dt * np.arange(len(g))))[2:])                 # t[i] against t0 + i dt
        assert off.min() > 0.1 * abs(dt) and off.max() > abs(dt)
    assert C.GRIDS['decreasing'][1] < C.GRIDS['decreasing'][0]
    assert abs(C.MAIN[1] - C.MAIN[0] - 0.25) < 1e-15 and len(C.MAIN) == 9


def test_every_net_is_on_its_side_of_the_lds_budget():
    assert C.lds_bytes(C.BY_NAME['lds_exact']) == 163840 == C.LDS_BUDGET          # the whole LDS of a compute unit
    assert C.LDS_BUDGET - 16 * 1024 < C.lds_bytes(C.BY_NAME['lds_under']) < C.LDS_BUDGET
    assert C.LDS_BUDGET - 8 * 1024 < C.lds_bytes(C.BY_NAME['f32_lds_under']) < C.LDS_BUDGET
    for name, side in C.BUDGET.items():
        c = C.BY_NAME[name]
        assert C.path_of(c) == side, (name, C.lds_bytes(c))
        assert C.pack_elems(c) * np.dtype(c.dtype).itemsize <= C.WORKSPACE
    assert set(C.path_of(c) for c in F64) == set(C.path_of(c) for c in F32) == {'lds', 'l2'}
    six = C.BY_NAME['l2_six']
    assert len(six.hidden) + 1 == N.HYPER_MAX_LAYERS and C.pack_elems(six) * 8 > C.WORKSPACE // 2
    for c in C.CASES:                                           # every other case: in LDS
        if c.name not in C.BUDGET:
            assert C.path_of(c) == 'lds', c.name


def test_describe_g_accepts_every_net():
    for c in C.CASES:
        g = C.make_g(c)
        tab, why = H.describe_g(g, c.D)
        assert why is None, (c.name, why)
        assert len(tab['layers']) == len(c.hidden) + 1
        assert [lin.out_features for lin, _, _ in tab['layers']] == list(C.widths(c)[1:])
        assert all(p.dtype == getattr(torch, c.dtype) and not p.requires_grad for p in g.parameters())
        assert len(HR.g_layers(g)) == len(tab['layers'])
    assert any(isinstance(m, torch.nn.Identity) for m in C.make_g(C.BY_NAME['identity']))


def test_float32_cases_hold_float32_values_and_rows_do_not_depend_on_the_batch():
    for c in F32:
        for v in (C.grid_of(c), C.y0_of(c, 5), C.base_of(c) if c.B <= 64 else C.y0_of(c, 3)):
            assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
        for W, b, act, a in C.layers_of(c):
            assert np.array_equal(W, W.astype(np.float32).astype(np.float64))
            if act == 'leaky':
                assert a == float(np.float32(0.2))
    c = C.BY_NAME['w50_prelu1']
    assert np.array_equal(C.y0_of(c)[[0, 15, 16, 36]], np.concatenate([C.y0_of(c, 1), C.y0_of(c, 37)[[15, 16, 36]]]))
    big = C.BY_NAME['trip2']
    assert np.array_equal(C.y0_of(big)[:37], C.y0_of(big, 37))


@pytest.mark.parametrize('case', SMALL, ids=lambda c: c.name)
def test_every_wrong_variant_is_visible_at_100_bounds(case):
    for op in case.ops:
        ref = C.reference(case, op)
        assert np.isfinite(ref).all() and np.abs(ref).max() < 1e3
        bound = C.bound_of(case, op)
        for v in C.variants_of(case, op):
            d = bands.observed(C.wrong(case, op, v), ref)
            assert d > 100 * bound, '%s %s: the defect %s moves the result by %.3e, the bound is %.3e' % (case.name, op, v, d, bound)


def test_which_variants_apply():
    c = C.BY_NAME['w50_prelu1']
    assert C.variants_of(c, 'euler') == ['t0', 'local_dt', 'g0']
    assert C.variants_of(c, 'midpoint') == C.variants_of(c, 'heun') == ['t0', 'dt2', 'stage_time', 'local_dt', 'g0']
    assert C.variants_of(c, 'resid') == ['t0'] and C.variants_of(c, 'gresid') == ['t0', 'g0']
    assert 't0' not in C.variants_of(C.BY_NAME['lotka'], 'heun')            # autonomous
    two = C.BY_NAME['two_times']
    assert C.variants_of(two, 'euler') == ['g0'] and 'local_dt' not in C.variants_of(two, 'heun') and 't0' in C.variants_of(two, 'heun')


@pytest.mark.parametrize('case', [c for c in SMALL if any(a not in (None, 'tanh') for a in c.acts)], ids=lambda c: c.name)
def test_the_activations_reach_both_branches(case):
    for op in [o for o in case.ops if o != 'resid']:
        pre = []
        C.restate(case, op, pre=pre)
        per_layer = {}
        n = len(case.acts)
        for j, (act, z) in enumerate(pre):
            per_layer.setdefault(j % n, []).append(z)
        for l, zs in per_layer.items():
            z = np.concatenate([v.ravel() for v in zs])
            act = case.acts[l]
            if act in ('relu', 'leaky', 'prelu', 'prelu1'):
                assert (z > 0.05).sum() >= 10 and (z < -0.05).sum() >= 10, (case.name, op, l)
            if act == 'softplus' and case.first_scale > 1:
                assert (z > 20.5).sum() >= 10 and ((z > 1) & (z < 19.5)).sum() >= 10 and (z < -30).sum() >= 10, (case.name, op, l)


@pytest.mark.parametrize('case', F32, ids=lambda c: c.name)
def test_float32_bounds_follow_the_scheme_and_stay_below_1e_4(case):
    for op in case.ops:
        e = C.e32(case, op)
        floor = bands.case_ceiling(C.steps_of(case, op), stages=C.G_EVALS[op])
        b = C.bound_of(case, op)
        assert np.isfinite(e) and b == 4 * max(e, floor) and 1.6e-5 <= b < 1e-4, (case.name, op, e, b)
        if case.system == 'forced' and case.first_scale == 1:   # (E32 1e-7 .. 5e-7 on the oscillator: the floor decides)
            assert e < 1e-6 and b == 4 * floor


def test_float32_restatement_agrees_with_torch_float32_eager():
    """The float32 restatement against the package's eager loop (torch operations, the reference's formulas) on the CPU in float32: two
    float32 evaluations of the same formulas, apart by library roundings only - held to the a-priori ceiling of one comparison."""
    for name in ('f32_l4_mixed', 'f32_ring8'):
        case = C.BY_NAME[name]
        f, opts = C.make_f(case)
        g = C.make_g(case)
        t = torch.tensor(C.grid_of(case), dtype=torch.float32)
        y0 = torch.tensor(C.y0_of(case), dtype=torch.float32)
        for op, cls in (('euler', H.HyperEuler), ('midpoint', H.HyperMidpoint), ('heun', H.HyperHeun)):
            s = cls(f, g, options=opts)
            eager = s._eager(N.HYPER_TRAJECTORY, t, y0)
            assert eager.dtype == torch.float32
            mine = C.restate(case, op, dtype='float32')
            assert mine.dtype == np.float32
            assert bands.observed(eager.numpy(), mine) <= bands.case_ceiling(C.steps_of(case, op), stages=C.G_EVALS[op])
        base = torch.tensor(C.base_of(case), dtype=torch.float32)
        s = H.HyperEuler(f, g, options=opts)
        assert bands.observed(s._eager(N.HYPER_RESIDUAL, t, base).numpy(), C.restate(case, 'resid', dtype='float32')) <= 4 * C.e32(case, 'resid') + 4e-6
        assert bands.observed(s._eager(N.HYPER_G_RESIDUALS, t, base).numpy(), C.restate(case, 'gresid', dtype='float32')) <= 4e-6


def test_float64_restatement_agrees_with_torch_float64_eager():
    for name in ('l6_mixed', 'ring17', 'w127_softplus', 'cubic2', 'linear2', 'lotka'):
        case = C.BY_NAME[name]
        f, opts = C.make_f(case)
        g = C.make_g(case)
        t, y0 = torch.tensor(C.grid_of(case)), torch.tensor(C.y0_of(case))
        for op, cls in (('euler', H.HyperEuler), ('midpoint', H.HyperMidpoint), ('heun', H.HyperHeun)):
            eager = cls(f, g, options=opts)._eager(N.HYPER_TRAJECTORY, t, y0)
            assert bands.observed(eager.numpy(), C.reference(case, op)) <= 1e-13
