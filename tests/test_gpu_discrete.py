"""GPU tests of tfdiffeq_amd.discrete: the fused one-launch reverse sweep and the generic sweep against autograd through the float64 CPU
restatement of the same discrete map (tests/discrete_restatement.py).

Metric, per gradient tensor: max|got - ref| / max|ref|.  Ceiling: bands.case_ceiling(attempts=n_steps, stages=2 x stages of the method)
for float32 (forward plus transposed evaluation per stage), the same expression with eps64 and the floor scaled by 2^-29 for float64.
Every float32 case also asserts that the float32 CPU restatement itself is inside the ceiling (the inputs are ones the reference passes).
A relu network only is one when no sample crosses a kink between precisions: the gradient is discontinuous there, and ONE sample whose
pre-activation changes sign contributes 1e-4 .. 1e-3 in the metric.  Which samples cross depends on the rounding of each float32
implementation (the CPU restatement and the kernel flip different ones: at batch 4096, rk4 on 21 grid points, 84 million pre-activations,
20 of them within 1e-7 of zero), so a seed that is lucky for one is not for the other.  The relu inputs are therefore built on the CPU
with a margin (kink_free_rows): rows are independent trajectories, and a row is kept only if every pre-activation of its float64
restatement is at least KINK_MARGIN from zero.  Observed values: profiles/discrete_gpu_tests.txt.
"""
import copy
import functools

import pytest
import torch

from tfdiffeq_amd import discrete, models, odeint, odeint_discrete
from tests import discrete_restatement as DR

pytestmark = pytest.mark.gpu

GRIDS = (('euler', 2), ('euler', 5), ('midpoint', 5), ('heun', 5), ('rk4', 2), ('rk4', 5), ('rk4', 21))
ACTS = ('tanh', 'softplus', 'relu')
BIG, SMALL = (64, 128), (16, 32)
# The distance every relu pre-activation of a kept row keeps from zero in the float64 restatement.  It comes from the reference's own
# error: over these cases the float32 CPU restatement's pre-activations are at most 1.9e-6 from the float64 ones (rms 1e-7); twice that.
KINK_MARGIN = 4e-6


def case_list():
    cases = [(BIG, 4096, m, n, a) for m, n in GRIDS for a in ACTS]
    cases += [(BIG, 1000, m, n, 'tanh') for m, n in GRIDS] + [(BIG, 1000, 'rk4', 5, a) for a in ('softplus', 'relu')]
    cases += [(SMALL, 200, m, n, a) for m, n in (('euler', 2), ('heun', 5), ('rk4', 5)) for a in ACTS]
    return cases


def kink_free_rows(func, y0, t, method, batch):
    """The first `batch` rows of y0 whose float64 restatement keeps every pre-activation (the outputs of fc1 and fc2 at every stage of
    every step) at least KINK_MARGIN from zero."""
    f64 = copy.deepcopy(func).double()
    worst = torch.full((y0.shape[0],), float('inf'), dtype=torch.float64)

    def note(module, inputs, out):
        worst.copy_(torch.minimum(worst, out.detach().abs().amin(dim=-1)))
    hooks = [m.register_forward_hook(note) for m in (f64.fc1, f64.fc2)]
    with torch.no_grad():
        DR.solve(f64, y0.double(), t.double(), method)
    for h in hooks:
        h.remove()
    keep = torch.nonzero(worst >= KINK_MARGIN).flatten()
    print('relu rows at least %.0e from every kink: %d of %d (%d wanted), %s N=%d' % (KINK_MARGIN, keep.numel(), y0.shape[0], batch, method, t.shape[0]))
    assert keep.numel() >= batch, 'only %d of %d rows keep %.1e from every kink' % (keep.numel(), y0.shape[0], KINK_MARGIN)
    return y0[keep[:batch]].contiguous()


def build(geom, batch, method, n, act, seed, time_dependent=False, t=None):
    """(float32 CPU network, y0, t, weights of the loss at every grid point) of a case.  t: the grid (its n points), default
    linspace(0, 1, n)."""
    torch.manual_seed(1000 + seed)
    func = models.ODEFunc(geom[0], geom[1], time_dependent=time_dependent, non_linearity=act)
    g = torch.Generator().manual_seed(2000 + seed)
    if t is None:
        t = torch.linspace(0., 1., n)
    assert t.shape[0] == n
    if act == 'relu':
        y0 = kink_free_rows(func, torch.randn(2 * batch, geom[0], generator=g), t, method, batch)
    else:
        y0 = torch.randn(batch, geom[0], generator=g)
    w = torch.randn(n, batch, geom[0], generator=g)
    return func, y0, t, w


def reference64(func, y0, t, w, method):
    """(y0 gradient, parameter gradients) of the float64 CPU restatement."""
    f64 = copy.deepcopy(func).double()
    _, gy, gp = DR.gradients(f64, tuple(f64.parameters()), y0.double(), t.double(), method, w.double())
    return gy + gp


def guard32(func, y0, t, w, method, ref, ceil, what):
    """The float32 CPU restatement's own deviation from the float64 one is inside the ceiling."""
    _, gy, gp = DR.gradients(func, tuple(func.parameters()), y0, t, method, w)
    worst = max(DR.rel_max(a, b) for a, b in zip(gy + gp, ref))
    print('%s: float32 CPU restatement vs float64: %.3e (ceiling %.3e)' % (what, worst, ceil))
    assert worst <= ceil, '%s: the float32 restatement itself is %.3e off its float64 twin (ceiling %.3e): not an input the reference passes' % (what, worst, ceil)
    return worst


def run_discrete(func_gpu, y0, t, w, method):
    for p in func_gpu.parameters():
        p.grad = None
    y = y0.clone().requires_grad_(True)
    sol = odeint_discrete(func_gpu, y, t, method=method)
    (sol * w).sum().backward()
    return sol.detach(), [y.grad] + [p.grad for p in func_gpu.parameters()], dict(odeint_discrete.last_backward_stats)


def compare(got, ref, ceil, what):
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        err = DR.rel_max(a, b)
        worst = max(worst, err)
        print('%s tensor %d: %.3e (ceiling %.3e)' % (what, i, err, ceil))
    assert worst <= ceil, '%s: max|got - ref| / max|ref| = %.3e above the ceiling %.3e' % (what, worst, ceil)
    return worst


@pytest.mark.parametrize('geom,batch,method,n,act', case_list())
def test_fused_sweep_float32(geom, batch, method, n, act):
    dev = torch.device('cuda:0')
    what = 'fused %dx%d b%d %s N=%d %s' % (geom + (batch, method, n, act))
    func, y0, t, w = build(geom, batch, method, n, act, 0)
    ref = reference64(func, y0, t, w, method)
    ceil = DR.ceiling32(n - 1, method)
    guard32(func, y0, t, w, method, ref, ceil, what)
    fg = copy.deepcopy(func).to(dev)
    _, got, stats = run_discrete(fg, y0.to(dev), t, w.to(dev), method)
    assert stats['engine'] == 'fused mlp sweep' and stats['n_launches'] == 1 and stats['n_steps'] == n - 1, stats
    compare(got, ref, ceil, what)
    _, again, _ = run_discrete(fg, y0.to(dev), t, w.to(dev), method)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), what + ': two identical calls differ in some bit'


# More than one 32-row tile per workgroup: 32768 + 40 rows are 1026 tiles, the last of 8 rows; on 256 workgroups two own 5 tiles and the
# others 4 (on any grid of at most 1024 workgroups the counts are unequal or above one).  CHUNK_TILES = 0 is "steps outer" (one
# weight-gradient pass over all of a workgroup's tiles per step), 1 "tiles outer" (the partial sums carried from chunk to chunk), 2 leaves
# the workgroups with 5 tiles a short last chunk.  The reference of a case is computed once and shared by the three schedules.
MANY = 32768 + 40


@functools.lru_cache(maxsize=None)
def many_tiles_case(method, n, act):
    func, y0, t, w = build(BIG, MANY, method, n, act, 0)
    ref = reference64(func, y0, t, w, method)
    what = 'fused 64x128 b%d %s N=%d %s' % (MANY, method, n, act)
    guard32(func, y0, t, w, method, ref, DR.ceiling32(n - 1, method), what)
    return func, y0, t, w, ref, what


@pytest.mark.parametrize('chunk', (0, 1, 2))
@pytest.mark.parametrize('method,n,act', (('rk4', 5, 'tanh'), ('euler', 2, 'relu')))
def test_fused_sweep_many_tiles_per_workgroup(monkeypatch, method, n, act, chunk):
    dev = torch.device('cuda:0')
    func, y0, t, w, ref, what = many_tiles_case(method, n, act)
    what += ' chunk=%d' % chunk
    monkeypatch.setattr(discrete, 'CHUNK_TILES', chunk)
    fg = copy.deepcopy(func).to(dev)
    _, got, stats = run_discrete(fg, y0.to(dev), t, w.to(dev), method)
    assert stats['engine'] == 'fused mlp sweep' and stats['n_launches'] == 1 and stats['n_steps'] == n - 1, stats
    eng = [e for k, e in discrete._ENGINES.items() if k[0] == MANY and k[-1] == chunk and k[3] == method][-1]
    assert eng.desc.chunk_tiles == chunk
    compare(got, ref, DR.ceiling32(n - 1, method), what)
    _, again, _ = run_discrete(fg, y0.to(dev), t, w.to(dev), method)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), what + ': two identical calls differ in some bit'


@pytest.mark.parametrize('geom,batch,method,n,act', case_list())
def test_generic_sweep_float64(geom, batch, method, n, act):
    dev = torch.device('cuda:0')
    what = 'generic f64 %dx%d b%d %s N=%d %s' % (geom + (batch, method, n, act))
    func, y0, t, w = build(geom, batch, method, n, act, 0)
    ref = reference64(func, y0, t, w, method)
    fg = copy.deepcopy(func).double().to(dev)
    _, got, stats = run_discrete(fg, y0.double().to(dev), t.double(), w.double().to(dev), method)
    assert stats['engine'] == 'generic sweep' and stats['why'], stats
    compare(got, ref, DR.ceiling64(n - 1, method), what)


def _check_generic(func_cpu64, params_of, y0, t, method, what, call=None):
    """A float64 case of any callable: CPU restatement against odeint_discrete on the GPU (generic sweep, `why` says why)."""
    dev = torch.device('cuda:0')
    tensor_input = isinstance(y0, torch.Tensor)
    ys = (y0,) if tensor_input else tuple(y0)
    n = t.shape[0]
    g = torch.Generator().manual_seed(77)
    w = tuple(torch.randn((n,) + tuple(y.shape), dtype=torch.float64, generator=g) for y in ys)
    _, gy, gp = DR.gradients(func_cpu64, params_of(func_cpu64), y0, t, method, w[0] if tensor_input else w)
    fg = copy.deepcopy(func_cpu64)
    fg = fg.to(dev) if isinstance(fg, torch.nn.Module) else fg
    pg = params_of(fg)
    yg = tuple(y.to(dev).requires_grad_(True) for y in ys)
    sol = (call or (lambda f, y_, t_: odeint_discrete(f, y_, t_, method=method)))(fg, yg[0] if tensor_input else yg, t)
    sol = (sol,) if isinstance(sol, torch.Tensor) else sol
    grads = torch.autograd.grad(sum((w_.to(dev) * s).sum() for w_, s in zip(w, sol)), yg + tuple(pg), allow_unused=True)
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == 'generic sweep' and stats['why'], stats
    print(what, 'why:', stats['why'])
    compare(list(grads), gy + gp, DR.ceiling64(n - 1, method), what)


@pytest.mark.parametrize('method,n', (('euler', 2), ('midpoint', 5), ('rk4', 5)))
def test_generic_sweep_other_functions(method, n):
    t = torch.linspace(0., 1., n, dtype=torch.float64)
    g = torch.Generator().manual_seed(5)
    mod_params = lambda f: tuple(f.parameters())             # noqa: E731
    torch.manual_seed(21)
    _check_generic(models.ODEFunc(16, 32, time_dependent=True, non_linearity='tanh').double(), mod_params,
                   torch.randn(200, 16, dtype=torch.float64, generator=g), t, method, 'time-dependent ODEFunc')
    _check_generic(models.LinearODEFunc(16, dtype=torch.float64), mod_params, torch.randn(200, 16, dtype=torch.float64, generator=g), t, method,
                   'LinearODEFunc')

    class Net(torch.nn.Module):                              # a two-component tuple state
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(4, 3).double()

        def forward(self, t_, y):
            a, b = y
            return (torch.tanh(self.lin(b)) - 0.3 * a, torch.sin(a).sum(-1, keepdim=True) * b * 0.2)
    _check_generic(Net(), mod_params, (torch.randn(50, 3, dtype=torch.float64, generator=g), torch.randn(50, 4, dtype=torch.float64, generator=g)),
                   t, method, 'tuple state')


@pytest.mark.parametrize('method,n', (('euler', 2), ('rk4', 5)))
def test_generic_sweep_lowered_style_lambda(method, n):
    """A plain callable over closed-over trainable tensors, of the shape the tracer lowers (matmul, tanh, elementwise)."""
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(6)
    A0, b0 = 0.4 * torch.randn(8, 8, dtype=torch.float64, generator=g), 0.1 * torch.randn(8, dtype=torch.float64, generator=g)
    y0 = torch.randn(300, 8, dtype=torch.float64, generator=g)
    t = torch.linspace(0., 1., n, dtype=torch.float64)
    w = torch.randn(n, 300, 8, dtype=torch.float64, generator=g)
    A, b = A0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    _, gy, gp = DR.gradients(lambda t_, y: torch.tanh(y @ A + b) - 0.5 * y, (A, b), y0, t, method, w)
    Ag, bg = A0.to(dev).requires_grad_(True), b0.to(dev).requires_grad_(True)
    yg = y0.to(dev).requires_grad_(True)
    sol = odeint_discrete(lambda t_, y: torch.tanh(y @ Ag + bg) - 0.5 * y, yg, t, method=method)
    grads = torch.autograd.grad((sol * w.to(dev)).sum(), (yg, Ag, bg))
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == 'generic sweep' and stats['why'], stats
    compare(list(grads), gy + gp, DR.ceiling64(n - 1, method), 'lambda %s N=%d' % (method, n))


@pytest.mark.parametrize('solver', ('euler', 'rk4'))
def test_conv_block_discrete(solver):
    dev = torch.device('cuda:0')
    torch.manual_seed(8)
    func = models.Conv2dODEFunc(3, 8, non_linearity='softplus').double()
    x = torch.randn(4, 3, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    t = torch.tensor([0., 1.], dtype=torch.float64)
    w = torch.randn(2, 4, 3, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(10))
    _, gy, gp = DR.gradients(func, tuple(func.parameters()), x, t, solver, w)
    block = models.ODEBlock(copy.deepcopy(func).to(dev), is_conv=True, solver=solver, gradient='discrete')
    xg = x.to(dev).requires_grad_(True)
    out = block(xg)                                          # the state at t = 1
    grads = torch.autograd.grad((out * w[1].to(dev)).sum(), (xg,) + tuple(block.odefunc.parameters()))
    # (the restatement's loss also weighs the state at t = 0, which is x itself: its gradient there is w[0])
    ref = [gy[0] - w[0]] + gp
    stats = dict(odeint_discrete.last_backward_stats)
    assert stats['engine'] == 'generic sweep' and stats['why'], stats
    compare(list(grads), ref, DR.ceiling64(1, solver), 'conv block %s' % solver)


def _block_grads(block, x, w1):
    for p in block.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    (block(xg) * w1).sum().backward()
    return [xg.grad] + [p.grad for p in block.odefunc.parameters()]


def test_discrete_and_adjoint_gradients_differ_on_one_euler_step():
    """The distinction cannot collapse silently: with one Euler step over [0, 1] the discrete gradient is the taped one, the default route
    (the continuous adjoint, unchanged) is O(h) away from it - more than 1e-2 in the same metric (0.22 in a CPU proxy of the tanh case)."""
    dev = torch.device('cuda:0')
    func, y0, t, w = build(BIG, 4096, 'euler', 2, 'tanh', 0)
    ref = reference64(func, y0, t, w, 'euler')
    ref = [ref[0] - w[0].double()] + ref[1:]               # ODEBlock returns the state at t = 1 only
    ceil = DR.ceiling32(1, 'euler')
    fg = copy.deepcopy(func).to(dev)
    disc = _block_grads(models.ODEBlock(fg, solver='euler', gradient='discrete'), y0.to(dev), w[1].to(dev))
    assert odeint_discrete.last_backward_stats['engine'] == 'fused mlp sweep'
    compare(disc, ref, ceil, 'ODEBlock euler gradient=discrete')
    default = _block_grads(models.ODEBlock(fg, solver='euler'), y0.to(dev), w[1].to(dev))
    gap = max(DR.rel_max(a, b) for a, b in zip(default, ref))
    print('ODEBlock euler default route vs the taped gradient: %.3e' % gap)
    assert gap > 1e-2, 'the default route is %.3e from the taped gradient: the two gradients have collapsed' % gap


def test_odenet_three_sgd_steps_match_the_taped_loop():
    """Three SGD steps of ODENet(gradient='discrete', solver='euler') against the same steps taken with the taped torch loop on the GPU,
    float32 both.  Metric: max|w - w_ref| / max|w_ref - w_initial| per tensor - the float32 ceiling applied to the weight update; three
    solves of one step each: case_ceiling(attempts=3, stages=2).
    Both loops store their weights in float32, so each step resolves a weight to eps32 |w| and the update to eps32 |w| / |w - w_initial|:
    the learning rate is large enough for the update to be resolved inside the ceiling (at 0.05 the updates are 3e-4 .. 7e-3 of weights
    of 0.12, and the float32 taped loop on the CPU is itself 3e-5 from its float64 twin; at 2.0 they are 6e-3 .. 0.17, the loss still
    falls 1.37, 1.01, 0.93).  As in the other float32 cases the CPU restatement's own deviation is asserted first."""
    dev = torch.device('cuda:0')
    torch.manual_seed(31)
    net = models.ODENet(64, 128, 10, non_linearity='tanh', solver='euler', gradient='discrete').to(dev)
    ref = copy.deepcopy(net)
    init = [p.detach().clone() for p in net.parameters()]
    g = torch.Generator().manual_seed(32)
    x, target = torch.randn(512, 64, generator=g).to(dev), torch.randn(512, 10, generator=g).to(dev)
    t = torch.tensor([0., 1.])
    lr = 2.0
    from tests import bands
    ceil = bands.case_ceiling(attempts=3, stages=2)
    cpu = []                                                 # the guard: the float32 taped loop on the CPU against its float64 twin
    for model, xc, tc in ((copy.deepcopy(ref).cpu().double(), x.cpu().double(), target.cpu().double()), (copy.deepcopy(ref).cpu(), x.cpu(), target.cpu())):
        for _ in range(3):
            for p in model.parameters():
                p.grad = None
            ((model.linear_layer(DR.solve(model.odeblock.odefunc, xc, t, 'euler')[1]) - tc) ** 2).mean().backward()
            with torch.no_grad():
                for p in model.parameters():
                    p -= lr * p.grad
        cpu.append([p.detach() for p in model.parameters()])
    guard = max(float((a.double() - b).abs().max() / (b - c.cpu().double()).abs().max()) for b, a, c in zip(cpu[0], cpu[1], init))
    print('ODENet SGD: float32 CPU taped loop vs float64: %.3e (ceiling %.3e)' % (guard, ceil))
    assert guard <= ceil, 'the float32 taped loop itself is %.3e of the update off its float64 twin (ceiling %.3e)' % (guard, ceil)
    for _ in range(3):
        for model, fwd in ((net, lambda m: m(x)), (ref, lambda m: m.linear_layer(DR.solve(m.odeblock.odefunc, x, t, 'euler')[1]))):
            for p in model.parameters():
                p.grad = None
            ((fwd(model) - target) ** 2).mean().backward()
            with torch.no_grad():
                for p in model.parameters():
                    p -= lr * p.grad
        assert odeint_discrete.last_backward_stats['engine'] == 'fused mlp sweep'
    worst = 0.0
    for i, (a, b, c) in enumerate(zip(net.parameters(), ref.parameters(), init)):
        err = float((a.detach() - b.detach()).abs().max() / (b.detach() - c).abs().max())
        worst = max(worst, err)
        print('ODENet SGD tensor %d: %.3e (ceiling %.3e)' % (i, err, ceil))
    assert worst <= ceil, 'weights after three SGD steps are %.3e of the update away from the taped loop (ceiling %.3e)' % (worst, ceil)


@pytest.mark.parametrize('method,n', (('euler', 2), ('heun', 5), ('rk4', 21)))
def test_forward_values_are_odeint_s(method, n):
    dev = torch.device('cuda:0')
    func, y0, t, _ = build(BIG, 1000, method, n, 'tanh', 0)
    fg = copy.deepcopy(func).to(dev)
    with torch.no_grad():
        want = odeint(fg, y0.to(dev), t, method=method)
    got = odeint_discrete(fg, y0.to(dev).requires_grad_(True), t, method=method)
    assert got.requires_grad and torch.equal(got.detach(), want)
    A = torch.randn(8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(dev).requires_grad_(True)
    f = lambda t_, y: torch.tanh(y @ A)                      # noqa: E731
    y8 = torch.randn(40, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        want = odeint(f, y8, t.double(), method=method)
    assert torch.equal(odeint_discrete(f, y8, t.double(), method=method).detach(), want)
