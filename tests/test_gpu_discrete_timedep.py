"""GPU tests of the fused one-launch reverse sweep for the TIME-DEPENDENT float32 ODEFunc (fc1 sees concat([t, x]); csrc/mi_ode_discrete.h
with a.td = 1), of the parameter subsets it now takes, and of the routes that must not have moved.

Reference and metric are those of tests/test_gpu_discrete.py: autograd through the float64 CPU restatement on the grid in the state dtype,
DR.rel_max per tensor, ceiling DR.ceiling32(n_steps, method); guard32 first in every case.  fc1.weight's gradient is compared as TWO
tensors - column 0 (w_t, the row that multiplies t) and columns 1.. - so that a missing time gradient cannot hide under the larger entries
of the same tensor, and every reference tensor is asserted nonzero.  No grid starts at 0 with one Euler step (the stage time would be 0
and the gradient of w_t identically zero): the grids are linspace(0.25, 1.75, n), linspace(1.0, -0.5, n) (decreasing: the network sees
the actual, decreasing times) and an uneven one from seeded random step widths starting at 0.5.

On the CPU, with build()'s seeds and these grids, the float32 restatement is 1.8e-7 .. 3.9e-7 from the float64 one over the cases below
(the w_t column alone 1.2e-7 .. 3.5e-7) under ceilings of 4e-6 .. 7.6e-5.
"""
import copy
import functools

import pytest
import torch

from tfdiffeq_amd import discrete, models, odeint_discrete
from tests import discrete_grid_restatement as DGR
from tests import discrete_restatement as DR
from tests.test_gpu_discrete import BIG, SMALL, build, compare, guard32, reference64, run_discrete

pytestmark = pytest.mark.gpu

FUSED = 'fused mlp sweep'


def grid_of(kind, n):
    if kind == 'shifted':
        return torch.linspace(0.25, 1.75, n)
    if kind == 'decreasing':
        return torch.linspace(1.0, -0.5, n)
    assert kind == 'uneven'
    widths = 0.1 + 0.4 * torch.rand(n - 1, generator=torch.Generator().manual_seed(4000 + n))
    return torch.cat([torch.tensor([0.5]), 0.5 + torch.cumsum(widths, 0)])


def split(grads):
    """[y0, fc1.weight, fc1.bias, ...] -> [y0, fc1.weight[:, :1] (the w_t column), fc1.weight[:, 1:], fc1.bias, ...]."""
    return [grads[0], grads[1][:, :1], grads[1][:, 1:]] + list(grads[2:])


def nonzero(ref, what):
    for i, r in enumerate(ref):
        assert float(r.abs().max()) > 0.0, '%s: reference tensor %d is identically zero: the case checks nothing there' % (what, i)


@functools.lru_cache(maxsize=None)
def case(geom, batch, method, n, act, grid):
    """(float32 CPU network, y0, t, w, float64 reference gradients (unsplit), ceiling, name) - built once, shared, never modified."""
    func, y0, t, w = build(geom, batch, method, n, act, 0, time_dependent=True, t=grid_of(grid, n))
    ref = reference64(func, y0, t, w, method)
    ceil = DR.ceiling32(n - 1, method)
    what = 'fused td %dx%d b%d %s N=%d %s %s' % (geom + (batch, method, n, act, grid))
    guard32(func, y0, t, w, method, ref, ceil, what)
    nonzero(split(ref), what)
    return func, y0, t, w, ref, ceil, what


CASES = (
    (SMALL, 200, 'euler', 2, 'relu', 'shifted'),             # 7 tiles, the last of 8 rows
    (SMALL, 200, 'rk4', 5, 'relu', 'decreasing'),
    (SMALL, 200, 'rk4', 21, 'tanh', 'shifted'),
    (BIG, 1000, 'rk4', 21, 'relu', 'shifted'),
    (BIG, 1000, 'rk4', 21, 'tanh', 'decreasing'),
    (BIG, 1000, 'heun', 5, 'relu', 'uneven'),
    (BIG, 1000, 'rk4', 5, 'tanh', 'uneven'),
    (BIG, 1000, 'midpoint', 5, 'softplus', 'decreasing'),
)


def fused_twice(func, y0, t, w, method, ref, ceil, what):
    """Route, parity per tensor (fc1.weight split) and bit-identical repetition of one fused call; returns the gradients."""
    dev = torch.device('cuda:0')
    fg = copy.deepcopy(func).to(dev)
    _, got, stats = run_discrete(fg, y0.to(dev), t, w.to(dev), method)
    assert stats['engine'] == FUSED and stats['n_launches'] == 1 and stats['n_steps'] == t.shape[0] - 1, stats
    compare(split(got), split(ref), ceil, what)
    _, again, _ = run_discrete(fg, y0.to(dev), t, w.to(dev), method)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), what + ': two identical calls differ in some bit'
    return got


@pytest.mark.parametrize('geom,batch,method,n,act,grid', CASES)
def test_fused_sweep_time_dependent(geom, batch, method, n, act, grid):
    func, y0, t, w, ref, ceil, what = case(geom, batch, method, n, act, grid)
    fused_twice(func, y0, t, w, method, ref, ceil, what)


# The partial of w_t is carried from chunk to chunk like every other accumulator: 32768 + 40 rows are 1026 tiles, the last of 8 rows, more
# than one per workgroup on any grid; CHUNK_TILES 0 / 1 / 2 as in test_fused_sweep_many_tiles_per_workgroup.  One shared reference.
MANY = 32768 + 40


@pytest.mark.parametrize('chunk', (0, 1, 2))
def test_chunk_carry_of_the_time_gradient(monkeypatch, chunk):
    func, y0, t, w, ref, ceil, what = case(BIG, MANY, 'rk4', 5, 'tanh', 'shifted')
    monkeypatch.setattr(discrete, 'CHUNK_TILES', chunk)
    fused_twice(func, y0, t, w, 'rk4', ref, ceil, what + ' chunk=%d' % chunk)
    eng = [e for k, e in discrete._ENGINES.items() if k[0] == MANY and k[-1] == chunk][-1]
    assert eng.desc.chunk_tiles == chunk and eng.time_dependent


def test_float64_grid_times_are_used_in_the_state_dtype():
    """`t` given in float64 with a float32 state: the same grid points, the same bits as the float32 `t`."""
    func, y0, t, w, ref, ceil, what = case(SMALL, 200, 'rk4', 5, 'relu', 'decreasing')
    dev = torch.device('cuda:0')
    fg = copy.deepcopy(func).to(dev)
    _, got, _ = run_discrete(fg, y0.to(dev), t, w.to(dev), 'rk4')
    _, got64, stats = run_discrete(fg, y0.to(dev), t.double(), w.to(dev), 'rk4')
    assert stats['engine'] == FUSED, stats
    assert all(torch.equal(a, b) for a, b in zip(got, got64))


# ---- own grid -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def own_grid_case():
    torch.manual_seed(41)
    func = models.ODEFunc(4, 8, time_dependent=True, non_linearity='tanh')
    g = torch.Generator().manual_seed(42)
    y0 = torch.randn(40, 4, generator=g)
    t, step = torch.tensor((0.5, 0.8, 1.15, 1.5)), 0.25                # grid 0.5, 0.75, 1.0, 1.25, 1.5: outputs 1 and 2 lie inside steps
    w = torch.randn(4, 40, 4, generator=g)
    f64 = copy.deepcopy(func).double()
    _, gy, gp = DGR.gradients(f64, tuple(f64.parameters()), y0.double(), t.double(), 'rk4', step, w.double(), time_dtype=torch.float32)
    ref = gy + gp
    _, gy32, gp32 = DGR.gradients(func, tuple(func.parameters()), y0, t, 'rk4', step, w)
    ceil = DR.ceiling32(4, 'rk4')
    guard = max(DR.rel_max(a, b) for a, b in zip(split(gy32 + gp32), split(ref)))
    print('own grid: float32 CPU restatement vs float64: %.3e (ceiling %.3e)' % (guard, ceil))
    assert guard <= ceil
    nonzero(split(ref), 'own grid')
    return func, y0, t, step, w, ref, ceil


@pytest.mark.parametrize('segments', (1, 2))
def test_own_grid_reaches_the_fused_sweep(monkeypatch, segments):
    """options['step_size'] with own_grid=True: the recompute on the grid, then the same kernel - each segment with its own times."""
    func, y0, t, step, w, ref, ceil = own_grid_case()
    dev = torch.device('cuda:0')
    if segments == 2:                                        # room for 3 grid points and their gradients: segments of 2 steps
        monkeypatch.setattr(discrete, 'GRID_BYTES', 2 * 3 * y0.numel() * y0.element_size())
    fg = copy.deepcopy(func).to(dev)
    y = y0.to(dev).requires_grad_(True)
    sol = odeint_discrete(fg, y, t, method='rk4', options={'step_size': step}, own_grid=True)
    assert sol.shape[0] == 4
    (sol * w.to(dev)).sum().backward()
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == FUSED and stats['n_steps'] == 4 and stats['n_launches'] == segments, stats
    assert stats['own_grid'] == {'n_grid_steps': 4, 'n_segments': segments, 'recompute_launches': 2 * segments - 1}, stats
    compare(split([y.grad] + [p.grad for p in fg.parameters()]), split(ref), ceil, 'own grid td, %d segment(s)' % segments)


# ---- ODEBlock / ODENet ----------------------------------------------------------------------------------------------------------------
def test_odeblock_on_a_shifted_grid():
    func, y0, t, w, ref, ceil, what = case(BIG, 1000, 'rk4', 5, 'tanh', 'uneven')
    dev = torch.device('cuda:0')
    block = models.ODEBlock(copy.deepcopy(func).to(dev), solver='rk4', gradient='discrete')
    x = y0.to(dev).requires_grad_(True)
    (block(x, eval_times=t) * w.to(dev)).sum().backward()
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == FUSED and stats['n_launches'] == 1 and stats['n_steps'] == 4, stats
    compare(split([x.grad] + [p.grad for p in block.odefunc.parameters()]), split(ref), ceil, 'ODEBlock td rk4')


def test_odenet_time_dependent_discrete():
    """ODENet(time_dependent=True, gradient='discrete', solver='rk4'): one rk4 step over [0, 1] (stage times 0, 1/3, 2/3, 1), the linear
    head on the state at t = 1.  The loss is a sum over a squared error; the odefunc's gradients against the float64 restatement."""
    dev = torch.device('cuda:0')
    torch.manual_seed(51)
    net = models.ODENet(16, 32, 10, time_dependent=True, non_linearity='tanh', solver='rk4', gradient='discrete')
    g = torch.Generator().manual_seed(52)
    x, target = torch.randn(200, 16, generator=g), torch.randn(200, 10, generator=g)
    t = torch.tensor([0., 1.])
    refs = []
    for model, xc, tc in ((copy.deepcopy(net).double(), x.double(), target.double()), (copy.deepcopy(net), x, target)):
        ((model.linear_layer(DR.solve(model.odeblock.odefunc, xc, t.to(xc.dtype), 'rk4')[1]) - tc) ** 2).sum().backward()
        refs.append([p.grad for p in model.odeblock.odefunc.parameters()] + [p.grad for p in model.linear_layer.parameters()])
    ceil = DR.ceiling32(1, 'rk4')
    ref, ref32 = ([r[0][:, :1], r[0][:, 1:]] + r[1:] for r in refs)
    guard = max(DR.rel_max(a, b) for a, b in zip(ref32, ref))
    print('ODENet td: float32 CPU restatement vs float64: %.3e (ceiling %.3e)' % (guard, ceil))
    assert guard <= ceil
    nonzero(ref, 'ODENet td')
    ng = copy.deepcopy(net).to(dev)
    ((ng(x.to(dev)) - target.to(dev)) ** 2).sum().backward()
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == FUSED and stats['n_launches'] == 1 and stats['n_steps'] == 1, stats
    got = [p.grad for p in ng.odeblock.odefunc.parameters()] + [p.grad for p in ng.linear_layer.parameters()]
    compare([got[0][:, :1], got[0][:, 1:]] + got[1:], ref, ceil, 'ODENet td rk4')


# ---- frozen parameters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('time_dependent', (True, False))
@pytest.mark.parametrize('frozen', ('fc2.bias', 'fc1.weight'))
def test_frozen_parameter_stays_on_the_fused_sweep(frozen, time_dependent):
    dev = torch.device('cuda:0')
    if time_dependent:
        func, y0, t, w, ref, ceil, what = case(SMALL, 200, 'rk4', 5, 'relu', 'decreasing')
    else:
        func, y0, t, w = build(SMALL, 200, 'rk4', 5, 'tanh', 0, t=grid_of('shifted', 5))
        ref, ceil, what = reference64(func, y0, t, w, 'rk4'), DR.ceiling32(4, 'rk4'), 'fused 16x32 b200 rk4 N=5 tanh shifted'
        guard32(func, y0, t, w, 'rk4', ref, ceil, what)
    fg = copy.deepcopy(func).to(dev)
    names = [n for n, _ in fg.named_parameters()]
    dict(fg.named_parameters())[frozen].requires_grad_(False)
    _, got, stats = run_discrete(fg, y0.to(dev), t, w.to(dev), 'rk4')
    assert stats['engine'] == FUSED and stats['n_launches'] == 1, stats
    k = 1 + names.index(frozen)
    assert got[k] is None, 'the frozen %s received a gradient' % frozen
    assert all(g_ is not None for i, g_ in enumerate(got) if i != k)
    keep = [i for i in range(len(got)) if i != k]
    if frozen == 'fc1.weight' or not time_dependent:
        compare([got[i] for i in keep], [ref[i] for i in keep], ceil, what + ' frozen ' + frozen)
    else:
        compare(split(got[:k]) + got[k + 1:], split(ref[:k]) + ref[k + 1:], ceil, what + ' frozen ' + frozen)


def test_a_tensor_outside_the_six_keeps_the_generic_sweep():
    func, y0, t, w, ref, ceil, what = case(SMALL, 200, 'rk4', 5, 'relu', 'decreasing')
    dev = torch.device('cuda:0')
    fg = copy.deepcopy(func).to(dev)
    fg.register_parameter('extra', torch.nn.Parameter(torch.zeros(3, device=dev)))
    _, got, stats = run_discrete(fg, y0.to(dev), t, w.to(dev), 'rk4')
    assert stats['engine'] == 'generic sweep' and 'extra parameters' in stats['why'], stats
    k = 1 + [n for n, _ in fg.named_parameters()].index('extra')
    assert got[k] is None                                    # (no step reaches the extra tensor)
    compare(split(got[:k] + got[k + 1:]), split(ref), ceil, what + ' + an extra parameter (generic)')


# ---- unchanged routes -----------------------------------------------------------------------------------------------------------------
def test_float64_time_dependent_net_keeps_the_generic_sweep():
    func, y0, t, w, ref, _, what = case(SMALL, 200, 'rk4', 5, 'relu', 'decreasing')
    dev = torch.device('cuda:0')
    fg = copy.deepcopy(func).double().to(dev)
    _, got, stats = run_discrete(fg, y0.double().to(dev), t.double(), w.double().to(dev), 'rk4')
    assert stats['engine'] == 'generic sweep' and 'float64' in stats['why'], stats
    compare(split(got), split(ref), DR.ceiling64(4, 'rk4'), what + ' float64 (generic)')


def test_time_independent_net_still_takes_the_fused_sweep():
    dev = torch.device('cuda:0')
    func, y0, t, w = build(SMALL, 200, 'rk4', 5, 'tanh', 0, t=grid_of('decreasing', 5))
    ref, ceil = reference64(func, y0, t, w, 'rk4'), DR.ceiling32(4, 'rk4')
    guard32(func, y0, t, w, 'rk4', ref, ceil, 'time independent')
    fg = copy.deepcopy(func).to(dev)
    _, got, stats = run_discrete(fg, y0.to(dev), t, w.to(dev), 'rk4')
    assert stats['engine'] == FUSED and stats['n_launches'] == 1 and stats['n_steps'] == 4, stats
    compare(got, ref, ceil, 'time independent')


def test_t_requiring_grad_still_raises():
    dev = torch.device('cuda:0')
    func = models.ODEFunc(4, 8, time_dependent=True, non_linearity='tanh').to(dev)
    t = torch.tensor([0.25, 1.0], requires_grad=True)
    with pytest.raises(ValueError, match='requires grad'):
        odeint_discrete(func, torch.randn(8, 4, device=dev), t, method='rk4')


@pytest.mark.parametrize('time_dependent', (True, False))
def test_tied_parameters_keep_the_generic_sweep(time_dependent):
    """fc2.bias IS fc1.bias: the module has five trainable tensors, all among the six slots, and the tied one's gradient is the sum of two
    of the kernel's.  The call stays on the generic sweep (as before the subset rule) and the sum is what it returns."""
    dev = torch.device('cuda:0')
    func, y0, t, w = build(SMALL, 200, 'rk4', 5, 'tanh', 0, time_dependent=time_dependent, t=grid_of('shifted', 5))
    func.fc2.bias = func.fc1.bias
    assert len(list(func.parameters())) == 5
    ref, ceil, what = reference64(func, y0, t, w, 'rk4'), DR.ceiling32(4, 'rk4'), 'tied biases td=%s' % time_dependent
    assert len(ref) == 6                                     # y0 and five tensors
    guard32(func, y0, t, w, 'rk4', ref, ceil, what)
    fg = copy.deepcopy(func).to(dev)
    assert fg.fc2.bias is fg.fc1.bias
    _, got, stats = run_discrete(fg, y0.to(dev), t, w.to(dev), 'rk4')
    assert stats['engine'] == 'generic sweep' and 'tied parameters' in stats['why'], stats
    compare(got, ref, ceil, what)
