"""GPU tests of the opt-in float64 fused mlp sweep (`discrete.MLP64` / `odeint_discrete(mlp64=...)`, csrc/mi_ode_discrete64.h).

Reference and metric are those of tests/test_gpu_discrete.py: autograd through the float64 CPU restatement (tests/discrete_restatement.py),
DR.rel_max per tensor, ceiling DR.ceiling64(n_steps, method) - the expression the float64 linear sweep and the float64 generic sweep are
held to; the tightest here is 7.45e-15, one Euler step.  There is no float32 guard: the reference is in the state's own dtype.  Relu inputs
come from build()'s kink_free_rows.  Every fused case asserts the engine name, n_steps, a bit-identical second call and that every
reference tensor is nonzero; a time-dependent net has fc1.weight's gradient split into its w_t column and the rest.  Every figure is printed
with its share of the ceiling: profiles/discrete_f64_gpu_tests.txt.
"""
import copy
import functools

import pytest
import torch

from tfdiffeq_amd import discrete, models, odeint_discrete
from tests import discrete_grid_restatement as DGR
from tests import discrete_restatement as DR
from tests.test_gpu_discrete import build, compare, reference64, run_discrete
from tests.test_gpu_discrete_geometry import _alternating
from tests.test_gpu_discrete_timedep import grid_of, nonzero, own_grid_case, split

pytestmark = pytest.mark.gpu

FUSED64 = 'fused mlp sweep (float64)'
OLD_WHY = 'dtype float64 (the fused sweep is float32)'


def grid64(kind, n):
    return torch.linspace(0., 1., n) if kind == 'linspace' else grid_of(kind, n)


@functools.lru_cache(maxsize=None)
def case(geom, batch, method, n, act, td, grid):
    """(float32-built CPU network, y0, t, w, float64 reference gradients (unsplit), ceiling, name) - built once, shared, never modified."""
    func, y0, t, w = build(geom, batch, method, n, act, 0, time_dependent=td, t=grid64(grid, n))
    ref = reference64(func, y0, t, w, method)
    what = 'fused f64 %dx%d b%d %s N=%d %s td=%d %s' % (geom + (batch, method, n, act, td, grid))
    nonzero(split(ref) if td else ref, what)
    return func, y0, t, w, ref, DR.ceiling64(n - 1, method), what


def shares(got, ref, ceil, what):
    for i, (a, b) in enumerate(zip(got, ref)):
        print('%s tensor %d: share of the ceiling %.3f' % (what, i, DR.rel_max(a, b) / ceil))
    return compare(got, ref, ceil, what)


def run64(fg, y0, t, w, method, monkeypatch, switch='auto'):
    dev = torch.device('cuda:0')
    monkeypatch.setattr(discrete, 'MLP64', switch)
    return run_discrete(fg, y0.double().to(dev), t.double(), w.double().to(dev), method)


def fused_twice(monkeypatch, func, y0, t, w, method, ref, ceil, what, td):
    fg = copy.deepcopy(func).double().to(torch.device('cuda:0'))
    _, got, stats = run64(fg, y0, t, w, method, monkeypatch)
    assert stats['engine'] == FUSED64 and stats['n_launches'] == 1 and stats['n_steps'] == t.shape[0] - 1 and stats['why'] == '', stats
    assert all(g.dtype == torch.float64 for g in got)
    shares(split(got) if td else got, split(ref) if td else ref, ceil, what)
    _, again, _ = run64(fg, y0, t, w, method, monkeypatch)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), what + ': two identical calls differ in some bit'
    return got


CASES = (
    ((16, 32), 200, 'rk4', 5, 'tanh', False, 'linspace'),       # the 64 x 128 kernel mostly padding; 7 tiles, the last of 8 rows
    ((16, 32), 200, 'euler', 2, 'relu', True, 'shifted'),       # one stage, the tightest ceiling, w_t
    ((64, 128), 1000, 'rk4', 21, 'relu', True, 'shifted'),      # full geometry, many steps
    ((64, 128), 1000, 'heun', 5, 'relu', True, 'uneven'),       # two-stage tableau, uneven h
    ((64, 128), 200, 'rk4', 5, 'softplus', False, 'linspace'),  # softplus' from the output
    ((64, 128), 1000, 'midpoint', 5, 'tanh', True, 'decreasing'),
    ((16, 16), 40, 'rk4', 5, 'relu', False, 'linspace'),        # the (16, 16) instantiation, two tiles
    ((5, 7), 33, 'midpoint', 5, 'tanh', True, 'decreasing'),    # (16, 16) ragged in both widths, a 1-row last tile
    ((48, 100), 65, 'rk4', 5, 'relu', True, 'uneven'),          # 64 x 128 ragged
    ((17, 16), 40, 'heun', 5, 'softplus', False, 'linspace'),   # dim just over the small box
)


@pytest.mark.parametrize('geom,batch,method,n,act,td,grid', CASES)
def test_fused_sweep_float64(monkeypatch, geom, batch, method, n, act, td, grid):
    func, y0, t, w, ref, ceil, what = case(geom, batch, method, n, act, td, grid)
    fused_twice(monkeypatch, func, y0, t, w, method, ref, ceil, what, td)


# 8192 + 40 rows are 258 tiles - more than one per workgroup on any grid of at most 256 - the last of 8 rows.  CHUNK_TILES 0 / 1 / 2 as
# in test_fused_sweep_many_tiles_per_workgroup: the partial sums (w_t's among them) are carried from chunk to chunk.  One shared reference.
MANY = 8192 + 40


@pytest.mark.parametrize('chunk', (0, 1, 2))
def test_chunk_carry(monkeypatch, chunk):
    func, y0, t, w, ref, ceil, what = case((64, 128), MANY, 'rk4', 5, 'tanh', True, 'shifted')
    monkeypatch.setattr(discrete, 'CHUNK_TILES', chunk)
    fused_twice(monkeypatch, func, y0, t, w, 'rk4', ref, ceil, what + ' chunk=%d' % chunk, True)
    eng = [e for k, e in discrete._ENGINES64.items() if k[0] == MANY and k[-1] == chunk][-1]
    assert eng.desc.chunk_tiles == chunk and eng.time_dependent


def test_1024_steps_stay_fused_and_1025_do_not(monkeypatch):
    dev = torch.device('cuda:0')
    t = _alternating(1024).double()
    func, y0, _, w = build((16, 16), 40, 'rk4', 1025, 'tanh', 0, t=_alternating(1024))
    f64 = copy.deepcopy(func).double()
    _, gy, gp = DR.gradients(f64, tuple(f64.parameters()), y0.double(), t, 'rk4', w.double())
    ref, ceil = gy + gp, DR.ceiling64(1024, 'rk4')
    nonzero(ref, '1024 steps')
    fg = copy.deepcopy(func).double().to(dev)
    monkeypatch.setattr(discrete, 'MLP64', 'auto')
    _, got, stats = run_discrete(fg, y0.double().to(dev), t, w.double().to(dev), 'rk4')
    assert stats['engine'] == FUSED64 and stats['n_steps'] == 1024 and stats['n_launches'] == 1, stats
    shares(got, ref, ceil, 'fused f64 16x16 b40 rk4 1024 alternating steps')
    _, again, _ = run_discrete(fg, y0.double().to(dev), t, w.double().to(dev), 'rk4')
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    t2 = _alternating(1025).double()
    g = torch.Generator().manual_seed(9)
    w2 = torch.randn(1026, 40, 16, dtype=torch.float64, generator=g)
    _, _, stats = run_discrete(fg, y0.double().to(dev), t2, w2.to(dev), 'rk4')
    assert stats['engine'] == 'generic sweep' and 'more than 1024 steps' in stats['why'], stats


@pytest.mark.parametrize('segments', (1, 2))
def test_own_grid_reaches_the_float64_sweep(monkeypatch, segments):
    func, y0, t, step, w, _, _ = own_grid_case()
    dev = torch.device('cuda:0')
    f64 = copy.deepcopy(func).double()
    _, gy, gp = DGR.gradients(f64, tuple(f64.parameters()), y0.double(), t.double(), 'rk4', step, w.double())
    ref, ceil = gy + gp, DR.ceiling64(4, 'rk4')
    nonzero(split(ref), 'own grid f64')
    if segments == 2:                                        # room for 3 grid points and their gradients: segments of 2 steps
        monkeypatch.setattr(discrete, 'GRID_BYTES', 2 * 3 * y0.numel() * 8)
    monkeypatch.setattr(discrete, 'MLP64', 'auto')
    fg = copy.deepcopy(func).double().to(dev)
    y = y0.double().to(dev).requires_grad_(True)
    sol = odeint_discrete(fg, y, t.double(), method='rk4', options={'step_size': step}, own_grid=True)
    (sol * w.double().to(dev)).sum().backward()
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == FUSED64 and stats['n_steps'] == 4 and stats['n_launches'] == segments, stats
    assert stats['own_grid'] == {'n_grid_steps': 4, 'n_segments': segments, 'recompute_launches': 2 * segments - 1}, stats
    shares(split([y.grad] + [p.grad for p in fg.parameters()]), split(ref), ceil, 'own grid f64 td, %d segment(s)' % segments)


def test_odenet_float64_follows_the_module_switch(monkeypatch):
    dev = torch.device('cuda:0')
    torch.manual_seed(51)
    net = models.ODENet(16, 32, 10, time_dependent=True, non_linearity='tanh', solver='rk4', gradient='discrete').double()
    g = torch.Generator().manual_seed(52)
    x, target = torch.randn(200, 16, generator=g).double(), torch.randn(200, 10, generator=g).double()
    t = torch.tensor([0., 1.], dtype=torch.float64)
    model = copy.deepcopy(net)
    ((model.linear_layer(DR.solve(model.odeblock.odefunc, x, t, 'rk4')[1]) - target) ** 2).sum().backward()
    r = [p.grad for p in model.odeblock.odefunc.parameters()] + [p.grad for p in model.linear_layer.parameters()]
    ref, ceil = [r[0][:, :1], r[0][:, 1:]] + r[1:], DR.ceiling64(1, 'rk4')
    nonzero(ref, 'ODENet f64')
    monkeypatch.setattr(discrete, 'MLP64', 'auto')
    ng = copy.deepcopy(net).to(dev)
    ((ng(x.to(dev)) - target.to(dev)) ** 2).sum().backward()
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == FUSED64 and stats['n_launches'] == 1 and stats['n_steps'] == 1, stats
    got = [p.grad for p in ng.odeblock.odefunc.parameters()] + [p.grad for p in ng.linear_layer.parameters()]
    shares([got[0][:, :1], got[0][:, 1:]] + got[1:], ref, ceil, 'ODENet f64 td rk4')


@pytest.mark.parametrize('frozen', ('fc2.bias', 'fc1.weight'))
def test_frozen_parameter_stays_fused(monkeypatch, frozen):
    func, y0, t, w, ref, ceil, what = case((16, 32), 200, 'rk4', 5, 'tanh', False, 'linspace')
    fg = copy.deepcopy(func).double().to(torch.device('cuda:0'))
    names = [n for n, _ in fg.named_parameters()]
    dict(fg.named_parameters())[frozen].requires_grad_(False)
    _, got, stats = run64(fg, y0, t, w, 'rk4', monkeypatch)
    assert stats['engine'] == FUSED64 and stats['n_launches'] == 1, stats
    k = 1 + names.index(frozen)
    assert got[k] is None, 'the frozen %s received a gradient' % frozen
    keep = [i for i in range(len(got)) if i != k]
    assert all(got[i] is not None for i in keep)
    shares([got[i] for i in keep], [ref[i] for i in keep], ceil, what + ' frozen ' + frozen)


def test_tied_parameters_keep_the_generic_sweep(monkeypatch):
    func, y0, t, w = build((16, 32), 200, 'rk4', 5, 'tanh', 0)
    func.fc2.bias = func.fc1.bias
    ref = reference64(func, y0, t, w, 'rk4')
    fg = copy.deepcopy(func).double().to(torch.device('cuda:0'))
    assert fg.fc2.bias is fg.fc1.bias
    _, got, stats = run64(fg, y0, t, w, 'rk4', monkeypatch)
    assert stats['engine'] == 'generic sweep' and 'tied parameters' in stats['why'], stats
    compare(got, ref, DR.ceiling64(4, 'rk4'), 'tied biases f64')


def test_float32_parameters_under_a_float64_state_keep_the_generic_sweep(monkeypatch):
    dev = torch.device('cuda:0')
    func, y0, t, w = build((16, 32), 200, 'rk4', 5, 'tanh', 0)

    class Mixed(models.ODEFunc):                              # float32 parameters, evaluated in the state's dtype
        def forward(self, t_, x):
            h = torch.tanh(x @ self.fc1.weight.t().double() + self.fc1.bias.double())
            h = torch.tanh(h @ self.fc2.weight.t().double() + self.fc2.bias.double())
            return h @ self.fc3.weight.t().double() + self.fc3.bias.double()
    fg = Mixed(16, 32, non_linearity='tanh')
    fg.load_state_dict(func.state_dict())
    fg = fg.to(dev)
    monkeypatch.setattr(discrete, 'MLP64', 'auto')
    y = y0.double().to(dev).requires_grad_(True)
    sol = odeint_discrete(fg, y, t.double(), method='rk4', _forward_func=lambda t_, x: fg(t_, x))
    (sol * w.double().to(dev)).sum().backward()
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == 'generic sweep' and 'parameters in another dtype' in stats['why'], stats


def test_mlp64_true_raises_at_the_call():
    dev = torch.device('cuda:0')
    func = models.ODEFunc(16, 129, non_linearity='tanh').double().to(dev)
    y = torch.randn(40, 16, dtype=torch.float64, device=dev).requires_grad_(True)
    with pytest.raises(ValueError, match='mlp64=True.*tile box'):
        odeint_discrete(func, y, torch.linspace(0., 1., 3, dtype=torch.float64), method='rk4', mlp64=True)


def test_switch_off_is_the_generic_sweep_with_the_old_words(monkeypatch):
    func, y0, t, w, ref, ceil, what = case((16, 32), 200, 'rk4', 5, 'tanh', False, 'linspace')
    fg = copy.deepcopy(func).double().to(torch.device('cuda:0'))
    assert discrete.MLP64 is False
    _, got, stats = run64(fg, y0, t, w, 'rk4', monkeypatch, switch=False)
    assert stats['engine'] == 'generic sweep' and stats['why'] == OLD_WHY, stats
    compare(got, ref, ceil, what + ' (switch off: generic)')


def test_float32_net_is_untouched_by_the_switch(monkeypatch):
    dev = torch.device('cuda:0')
    func, y0, t, w = build((16, 32), 200, 'rk4', 5, 'tanh', 0)
    fg = copy.deepcopy(func).to(dev)
    _, off, stats_off = run_discrete(fg, y0.to(dev), t, w.to(dev), 'rk4')
    monkeypatch.setattr(discrete, 'MLP64', 'auto')
    _, on, stats_on = run_discrete(fg, y0.to(dev), t, w.to(dev), 'rk4')
    assert stats_off['engine'] == stats_on['engine'] == 'fused mlp sweep', (stats_off, stats_on)
    assert all(torch.equal(a, b) for a, b in zip(off, on))
