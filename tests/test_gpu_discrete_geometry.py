"""GPU tests of the fused MLP reverse sweep (k_discrete_mlp<DP, HP, ACT>, csrc/mi_ode_discrete.h) over everything its host code dispatches
that tests/test_gpu_discrete.py does not reach: all four padded tile geometries x three activations (the twelve instantiations), ragged
widths, batches under one tile, uneven and decreasing grids, fewer parameters than workgroups, the 1024-step limit of the argument
block, what reaches _OdeintDiscrete.backward (leading batch axes, non-contiguous gradients and states, a loss on the last point) and the
engine cache.

The yardstick is that module's: autograd through the float64 CPU restatement (tests/discrete_restatement.py), the metric max|got - ref| /
max|ref| per gradient tensor, the ceilings DR.ceiling32 / DR.ceiling64 and the helpers build, reference64, guard32, kink_free_rows,
run_discrete and compare.  Every fused case: (a) the float32 CPU restatement is itself inside the ceiling (printed and asserted), (b) the
engine is the fused mlp sweep, one launch, len(t) - 1 steps, (c) all seven gradient tensors are inside the ceiling, (d) a second identical
call is bit-identical, (e) relu inputs come from kink_free_rows.  On top of that module's guard32 and compare, which fold the tensors with
max(), every per-tensor deviation must be a number and every reference gradient nonzero (0 / 0 would pass a max()).  The float64 reference sees the grid the solver sees: `t` in the state
dtype (float32), as the kernel's host code and the restatement form it.  Observed values: profiles/discrete_gpu_tests.txt.
"""
import contextlib
import copy
import functools
import io
import itertools
import math

import pytest
import torch

from tfdiffeq_amd import discrete, models, odeint, odeint_discrete
from tests import discrete_restatement as DR
from tests import test_gpu_discrete as TD

pytestmark = pytest.mark.gpu

ACTS = TD.ACTS
METHODS = ('euler', 'midpoint', 'heun', 'rk4')


def pad16(v, lo, hi):
    """The host code's choice of a padded width (csrc/mi_ode_discrete.hip)."""
    return lo if v <= lo else hi


def instantiation(geom):
    """(DP, HP) of the k_discrete_mlp instantiation mi_ode_discrete_create picks for (dim, hidden)."""
    return pad16(geom[0], 16, 64), pad16(geom[1], 16, 128)


# ---- grids ----------------------------------------------------------------------------------------------------------------------------
def _alternating(n_steps):
    """n_steps + 1 points from 0 with the widths 1.5/1024, 0.5/1024, 1.5/1024, ...: any wrong step index is an O(1) error in h."""
    widths = torch.tensor([1.5 / 1024, 0.5 / 1024], dtype=torch.float64).repeat((n_steps + 1) // 2)[:n_steps]
    return torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(widths, 0)]).float()


GRIDS = {
    'linspace5': lambda: torch.linspace(0., 1., 5),
    'linspace2': lambda: torch.linspace(0., 1., 2),
    'uneven': lambda: torch.tensor([0., .1, .35, .4, 1.]),
    'decreasing': lambda: torch.tensor([1., .6, .55, .2, 0.]),
    'uneven64': lambda: torch.tensor([0., .1, .35, .4, 1.], dtype=torch.float64),
    'alt1025': lambda: _alternating(1024),
    'alt1025flipped': lambda: _alternating(1024).flip(0).contiguous(),
    'alt1026': lambda: _alternating(1025),
}


class Case(object):
    """The CPU side of a case: network, inputs, float64 reference, ceiling, and the float32 CPU restatement's own deviation."""

    def __init__(self, geom, batch, method, act, grid, seed=0, last_only=False):
        t = GRIDS[grid]()
        self.geom, self.batch, self.method, self.act, self.n = geom, batch, method, act, int(t.shape[0])
        kernel = 'kernel %dx%d' % instantiation(geom) if geom[0] <= 64 and geom[1] <= 128 else 'outside the tile box'
        self.what = 'geometry %dx%d (%s) b%d %s %s %s' % (geom + (kernel, batch, method, grid, act))
        if seed:
            self.what += ' seed %d' % seed
        self.func, self.y0, self.t, self.w = TD.build(geom, batch, method, self.n, act, seed, t=t)
        if last_only:                                       # a loss on the last grid point alone
            self.what += ' loss on sol[-1]'
            self.w[:-1] = 0.
        self.ceil = DR.ceiling32(self.n - 1, method)
        self.refresh()

    def refresh(self):
        """(Re)compute the reference and the guard from the network's current weights."""
        # the discrete map lives on the grid in the state dtype (solvers.py:84): that is what the float64 reference differentiates
        self.ref = TD.reference64(self.func, self.y0, self.t.float(), self.w, self.method)
        # the metric divides by max|ref|: a tensor whose reference gradient is identically zero (a dead relu unit) would make it 0 / 0,
        # and max() / <= drop a nan silently - such an input is not a case: another seed
        for i, r in enumerate(self.ref):
            assert bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0., \
                '%s: the reference gradient of tensor %d is zero or not finite: change the seed' % (self.what, i)
        self.guard = guard32(self)
        self.shown = False                                  # the per-tensor lines of a case are printed by its first run only


def guard32(c):
    """Rule (a): TD.guard32 - the float32 CPU restatement's own deviation from the float64 one is inside the ceiling - with one more demand:
    the deviation of EVERY tensor is a number (TD.guard32 folds the tensors with max(), which passes over a nan)."""
    _, gy, gp = DR.gradients(c.func, tuple(c.func.parameters()), c.y0, c.t, c.method, c.w)
    devs = [DR.rel_max(a, b) for a, b in zip(gy + gp, c.ref)]
    assert all(math.isfinite(d) for d in devs), '%s: the float32 restatement\'s deviations are not all numbers: %s' % (c.what, devs)
    worst = max(devs)
    print('%s: float32 CPU restatement vs float64: %.3e (ceiling %.3e)' % (c.what, worst, c.ceil))
    assert worst <= c.ceil, '%s: the float32 restatement itself is %.3e off its float64 twin (ceiling %.3e): not an input the reference passes' % (c.what, worst, c.ceil)
    return worst


def compare(c, got):
    """Rule (c): TD.compare on all seven tensors, after asserting that every deviation is a number (TD.compare folds them with max(), which
    passes over a nan).  A case that several tests share prints its per-tensor lines the first time only."""
    devs = [DR.rel_max(a, b) for a, b in zip(got, c.ref)]
    assert len(devs) == 7 and all(math.isfinite(d) for d in devs), '%s: the deviations are not all numbers: %s' % (c.what, devs)
    with contextlib.redirect_stdout(io.StringIO()) if c.shown else contextlib.nullcontext():
        worst = TD.compare(got, c.ref, c.ceil, c.what)
    c.shown = True
    assert worst == max(devs)
    return worst


@functools.lru_cache(maxsize=None)
def case(geom, batch, method, act, grid, seed=0, last_only=False):
    return Case(geom, batch, method, act, grid, seed, last_only)


def fused(c, fg=None, y0=None, w=None, loss=None):
    """Rules (a) - (d) for the case c on cuda:0; returns (network on the GPU, forward solution, the seven gradients, worst deviation).
    y0 / w: the case's inputs in another shape or layout; loss: run_discrete's loss in another form."""
    dev = torch.device('cuda:0')
    assert math.isfinite(c.guard) and c.guard <= c.ceil     # (printed when the case was built)
    fg = copy.deepcopy(c.func).to(dev) if fg is None else fg
    y0 = c.y0.to(dev) if y0 is None else y0
    w = c.w.to(dev) if w is None else w
    run = TD.run_discrete if loss is None else loss
    sol, got, stats = run(fg, y0, c.t, w, c.method)
    assert stats['engine'] == 'fused mlp sweep' and stats['n_launches'] == 1 and stats['n_steps'] == c.n - 1, stats
    flat = [got[0].reshape(c.batch, c.geom[0])] + got[1:]
    worst = compare(c, flat)
    _, again, _ = run(fg, y0, c.t, w, c.method)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), c.what + ': two identical calls differ in some bit'
    print('%s: observed %.3e next to the float32 CPU restatement\'s %.3e' % (c.what, worst, c.guard))
    return fg, sol, flat, worst


def generic32(c, why_words):
    """A float32 case outside the fused kernel's scope: the generic sweep, `why` says why, gradients inside ceiling32."""
    dev = torch.device('cuda:0')
    assert math.isfinite(c.guard) and c.guard <= c.ceil     # (printed when the case was built)
    fg = copy.deepcopy(c.func).to(dev)
    _, got, stats = TD.run_discrete(fg, c.y0.to(dev), c.t, c.w.to(dev), c.method)
    assert stats['engine'] == 'generic sweep' and stats['n_steps'] == c.n - 1, stats
    print(c.what, 'why:', stats['why'])
    assert all(word in stats['why'] for word in why_words), stats['why']
    worst = compare(c, got)
    print('%s: observed %.3e next to the float32 CPU restatement\'s %.3e' % (c.what, worst, c.guard))


# ---- 1. geometry x activation ---------------------------------------------------------------------------------------------------------
# (dim, hidden) -> the instantiation it must select
GEOMETRIES = {
    (2, 16): (16, 16), (16, 16): (16, 16), (3, 5): (16, 16), (1, 1): (16, 16),
    (5, 17): (16, 128), (10, 100): (16, 128),
    (17, 16): (64, 16), (40, 12): (64, 16), (64, 16): (64, 16),
    (33, 50): (64, 128), (48, 96): (64, 128),
}


# Seeds other than build()'s 0.  (1, 1) relu: with seed 0 the single hidden unit is dead on every row - five of the seven reference
# gradients are identically zero and the metric is 0 / 0.
SEEDS = {((1, 1), 33, 'relu'): 8}


def geometry_cases():
    cases = [(g, 33, a) for g in GEOMETRIES for a in ACTS]                 # one full tile plus a one-row tile
    cases += [(g, 1, 'tanh') for g in GEOMETRIES]                          # grid = 1, 31 dead rows
    cases += [(g, 200, 'tanh') for g in GEOMETRIES if g != (1, 1)]         # ((1, 1) at 200 fails its own guard: one-element tensors)
    cases += [((64, 128), 1, 'softplus')]
    return cases


def test_parametrisation_covers_every_instantiation():
    """All four padded geometries x three activations - the twelve instantiations mi_ode_discrete.hip builds - are among the cases of
    test_geometry_and_activation, each at the batch of two tiles (33) at least."""
    want = set(itertools.product(((16, 16), (16, 128), (64, 16), (64, 128)), ACTS))
    for g, kernel in GEOMETRIES.items():
        assert instantiation(g) == kernel, (g, instantiation(g), kernel)
    have = set((instantiation(g), a) for g, b, a in geometry_cases() if b == 33)
    assert have == want, sorted(want - have)
    ragged = set(instantiation(g) for g in GEOMETRIES if g[0] % 16 and g[1] % 16)
    assert ragged == set(k for k, _ in want), 'a geometry without a case whose dim and hidden are both ragged'


@pytest.mark.parametrize('geom,batch,act', geometry_cases())
def test_geometry_and_activation(geom, batch, act):
    """Which instantiation ran is read off the shape with the host code's pad16 rule (the library does not report the template it
    launched): the assertion ties the case to the table above, it does not observe the kernel."""
    c = case(geom, batch, 'rk4', act, 'linspace5', SEEDS.get((geom, batch, act), 0))
    fused(c)
    assert instantiation(geom) == GEOMETRIES.get(geom, (64, 128))
    assert any(k[:3] == (batch, geom[0], geom[1]) for k in discrete._ENGINES), 'no engine of this shape was created'


# ---- 2. grids -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ('tanh', 'relu'))
@pytest.mark.parametrize('geom,batch', (((3, 5), 77), ((64, 128), 200)))
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('grid', ('uneven', 'decreasing'))
def test_uneven_and_decreasing_grids(grid, method, geom, batch, act):
    c = case(geom, batch, method, act, grid)
    fg, sol, _, _ = fused(c)
    with torch.no_grad():
        want = odeint(fg, c.y0.to(sol.device), c.t, method=method)
    assert torch.equal(sol, want), c.what + ': the forward values are not odeint\'s'


def test_float64_grid_with_a_float32_state():
    """`t` float64, the state float32: the kernel forms float(t[n + 1]) - float(t[n]), and so does the restatement."""
    c = case((3, 5), 77, 'rk4', 'tanh', 'uneven64')
    assert c.t.dtype == torch.float64 and c.y0.dtype == torch.float32
    fg, sol, got, _ = fused(c)
    with torch.no_grad():
        want = odeint(fg, c.y0.to(sol.device), c.t, method='rk4')
    assert torch.equal(sol, want)
    _, _, same, _ = fused(case((3, 5), 77, 'rk4', 'tanh', 'uneven'))       # the same grid, given in float32
    assert all(torch.equal(a, b) for a, b in zip(got, same))


# ---- 3. fewer parameters than workgroups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch,method,grid,act', ((2048, 'euler', 'linspace2', 'tanh'), (4096, 'rk4', 'linspace5', 'softplus'),
                                                   (4096, 'rk4', 'linspace5', 'relu')))
def test_fewer_parameters_than_workgroups(batch, method, grid, act):
    """ODEFunc(2, 3) has P = 29 parameters: with SL = ceil(P / grid) = 1 most workgroups own an empty slice of theta.
    The number of workgroups is computed here as the host code computes it, min(ceil(B / 32), compute units) (it also clamps to
    kPersistMaxGrid, 1024, far above both); the launch's real grid is not read back, so "most slices empty" is inferred, not measured."""
    P = 2 * 3 + 3 + 3 * 3 + 3 + 3 * 2 + 2
    workgroups = min((batch + 31) // 32, torch.cuda.get_device_properties(0).multi_processor_count)
    if workgroups <= P:
        pytest.skip('the launch has %d workgroups on this device, not more than the %d parameters' % (workgroups, P))
    c = case((2, 3), batch, method, act, grid)
    assert sum(r.numel() for r in c.ref[1:]) == P
    fused(c)


# ---- 4. the step limit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom,batch,method,act,grid', (((2, 16), 32, 'rk4', 'tanh', 'alt1025'), ((2, 16), 32, 'euler', 'relu', 'alt1025'),
                                                        ((17, 5), 40, 'heun', 'softplus', 'alt1025flipped')))
def test_1024_steps_are_fused(geom, batch, method, act, grid):
    """The whole h[] array of the argument block, alternating widths.  The ceiling is loose here (1e-3 .. 4e-3): the observed deviation
    is printed next to the float32 CPU restatement's (1.6e-6 .. 3.3e-6), so that a jump of orders of magnitude shows in the log."""
    c = case(geom, batch, method, act, grid)
    assert c.n == 1025
    h = c.t[1:] - c.t[:-1]
    flipped = grid.endswith('flipped')
    assert bool((h < 0).all()) if flipped else bool((h > 0).all())
    widths = h.abs().flip(0) if flipped else h               # in the order the grid was built
    assert float((widths[0::2] - 1.5 / 1024).abs().max()) < 1e-6 and float((widths[1::2] - 0.5 / 1024).abs().max()) < 1e-6
    fused(c)


def test_1025_steps_take_the_generic_sweep():
    c = case((2, 16), 32, 'euler', 'tanh', 'alt1026')
    assert c.n == 1026
    generic32(c, ('1024 steps',))


# ---- 5. what reaches backward ---------------------------------------------------------------------------------------------------------
def _backward_case():
    return case((10, 100), 100, 'rk4', 'tanh', 'linspace5')


def test_leading_batch_axes():
    c = _backward_case()
    dev = torch.device('cuda:0')
    _, _, flat, _ = fused(c)
    _, _, got, _ = fused(c, y0=c.y0.to(dev).reshape(4, 25, 10), w=c.w.to(dev).reshape(5, 4, 25, 10))
    assert all(torch.equal(a, b) for a, b in zip(got, flat)), 'a [4, 25, 10] state and its flat [100, 10] twin differ in some bit'


def test_non_contiguous_incoming_gradient():
    c = _backward_case()
    seen = []

    def permuted_loss(func_gpu, y0, t, w, method):
        for p in func_gpu.parameters():
            p.grad = None
        y = y0.clone().requires_grad_(True)
        sol = odeint_discrete(func_gpu, y, t, method=method)
        sol.register_hook(lambda g: seen.append(g.is_contiguous()))
        (sol.permute(1, 0, 2) * w.permute(1, 0, 2).contiguous()).sum().backward()
        return sol.detach(), [y.grad] + [p.grad for p in func_gpu.parameters()], dict(odeint_discrete.last_backward_stats)
    _, _, flat, _ = fused(c)
    _, _, got, _ = fused(c, loss=permuted_loss)
    assert seen and not any(seen), 'the incoming gradient was contiguous: the case does not test what it says'
    assert all(torch.equal(a, b) for a, b in zip(got, flat)), 'a non-contiguous incoming gradient changes some bit'


def test_non_contiguous_state():
    c = _backward_case()
    dev = torch.device('cuda:0')
    wide = torch.zeros(100, 20, device=dev)
    wide[:, 3:13] = c.y0.to(dev)
    seen = []

    def sliced_loss(func_gpu, y0, t, w, method):
        for p in func_gpu.parameters():
            p.grad = None
        y = y0.detach().requires_grad_(True)                 # (run_discrete's clone() would make it contiguous)
        seen.append(y.is_contiguous())
        sol = odeint_discrete(func_gpu, y, t, method=method)
        (sol * w).sum().backward()
        return sol.detach(), [y.grad] + [p.grad for p in func_gpu.parameters()], dict(odeint_discrete.last_backward_stats)
    _, sol_flat, flat, _ = fused(c)
    _, sol, got, _ = fused(c, y0=wide[:, 3:13], loss=sliced_loss)
    assert seen and not any(seen), 'the state was contiguous: the case does not test what it says'
    assert torch.equal(sol, sol_flat)
    assert all(torch.equal(a, b) for a, b in zip(got, flat)), 'a non-contiguous y0 and its contiguous copy differ in some bit'


def test_loss_on_the_last_point_alone():
    """Zero gradient at every interior grid point (and at t[0]): the reference is the restatement with those weights zeroed."""
    c = case((10, 100), 100, 'rk4', 'tanh', 'linspace5', 0, True)
    assert float(c.w[:-1].abs().max()) == 0. and float(c.w[-1].abs().max()) > 0.

    def last_point_loss(func_gpu, y0, t, w, method):
        for p in func_gpu.parameters():
            p.grad = None
        y = y0.clone().requires_grad_(True)
        sol = odeint_discrete(func_gpu, y, t, method=method)
        (sol[-1] * w[-1]).sum().backward()
        return sol.detach(), [y.grad] + [p.grad for p in func_gpu.parameters()], dict(odeint_discrete.last_backward_stats)
    fused(c, loss=last_point_loss)


# ---- 6. the engine cache --------------------------------------------------------------------------------------------------------------
def test_engine_cache_cycles_past_four_shapes():
    discrete.clear_engines()
    try:
        first = None
        for geom, batch in (((2, 16), 33), ((3, 5), 33), ((5, 17), 33), ((17, 16), 33), ((33, 50), 33), ((2, 16), 33)):
            _, _, got, _ = fused(case(geom, batch, 'rk4', 'tanh', 'linspace5'))
            assert 1 <= len(discrete._ENGINES) <= 4, list(discrete._ENGINES)
            assert any(k[:3] == (batch, geom[0], geom[1]) for k in discrete._ENGINES)
            first = got if first is None else first
        assert not any(k[:3] == (33, 3, 5) for k in discrete._ENGINES), 'the oldest engine was not the one evicted'
        assert all(torch.equal(a, b) for a, b in zip(got, first)), 'the first shape, after its engine was evicted and rebuilt, differs in some bit'
    finally:
        discrete.clear_engines()
    assert len(discrete._ENGINES) == 0


def test_two_networks_alternate_on_one_engine():
    """The engine is keyed on the shape, not on the activation or the weights: two networks of one shape share it."""
    a, b = case((2, 16), 33, 'rk4', 'tanh', 'linspace5'), case((2, 16), 33, 'rk4', 'softplus', 'linspace5', 1)
    assert not torch.equal(a.func.fc2.weight, b.func.fc2.weight)
    # the rest of the key - method, grid points, device, CHUNK_TILES - is the same for both, so they meet on ONE engine
    assert (a.batch, a.geom, a.method, a.n) == (b.batch, b.geom, b.method, b.n)
    discrete.clear_engines()
    try:
        nets, firsts = {}, {}
        for c in (a, b, a, b):
            nets[c], _, got, _ = fused(c, fg=nets.get(c))
            assert len(discrete._ENGINES) == 1, list(discrete._ENGINES)
            firsts.setdefault(c, got)
            assert all(torch.equal(x, y) for x, y in zip(got, firsts[c])), c.what + ': differs after the other network used the engine'
    finally:
        discrete.clear_engines()


def test_in_place_weight_update_between_calls():
    c = Case((2, 16), 33, 'rk4', 'tanh', 'linspace5')       # (its own copy: the weights change)
    fg, _, before, _ = fused(c)
    g = torch.Generator().manual_seed(41)
    with torch.no_grad():
        for p_cpu, p_gpu in zip(c.func.parameters(), fg.parameters()):
            p_cpu.add_(0.1 * torch.randn(p_cpu.shape, generator=g))
            p_gpu.copy_(p_cpu)                              # in place: the same storage, the same module
    c.what += ' after an in-place update'
    c.refresh()
    _, _, after, _ = fused(c, fg=fg)
    assert all(DR.rel_max(x, y) > 100 * c.ceil for x, y in zip(after, before)), 'the update did not move the gradients: the case tests nothing'


# ---- 7. the edge of the box -----------------------------------------------------------------------------------------------------------
def test_the_largest_box_is_fused():
    c = case((64, 128), 33, 'rk4', 'tanh', 'linspace5')
    assert instantiation(c.geom) == (64, 128)
    fused(c)


@pytest.mark.parametrize('geom', ((65, 16), (16, 129)))
def test_one_past_the_box_takes_the_generic_sweep(geom):
    generic32(case(geom, 33, 'rk4', 'tanh', 'linspace5'), ('tile box',))
