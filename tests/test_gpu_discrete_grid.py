"""GPU tests of odeint_discrete(own_grid=True): the one-launch linear kernel that recomputes its checkpoints (the GRID = true instantiations of
csrc/mi_ode_discrete_linear.h) and the recompute-on-the-grid route of the other engines, against autograd through the float64 CPU
restatement of the same solve (tests/discrete_grid_restatement.py: the step-size grid, the output loop, the linear interpolation).

Metric, per gradient tensor: DR.rel_max = max|got - ref| / max|ref|.  Ceilings: DR.ceiling64(n_grid_steps, method) for float64 and
DR.ceiling32(n_grid_steps, method) for float32 - the ones of tests/test_gpu_discrete_linear.py with the grid's step count.  The float64
reference of a float32 case walks the float32 case's grid (its points are exact in float64).  Each comparison prints its figure and its
share of the ceiling ("ratio"); observed values: profiles/discrete_grid_gpu_tests.txt.
"""
import copy
import functools

import pytest
import torch

from tfdiffeq_amd import discrete, models, odeint_discrete
from tests import discrete_grid_restatement as DGR
from tests import discrete_lowered_cases as DC
from tests import discrete_restatement as DR

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
# (t, step_size): a dyadic step - the hit at 0.25 is exact, two outputs share (0.25, 0.5], (0.5, 0.75] is empty; a clipped last step; a
# step larger than the span - one clipped step (no recomputation at all) with every output interpolated inside it
PAIRS = {'dyadic': ((0., 0.25, 0.3, 0.4, 1.0), 0.25), 'clipped': ((0., 0.35, 0.7, 1.0), 0.3), 'one_step': ((0., 0.5, 1.0), 2.0)}
KERNEL = 'fused linear sweep (own grid)'


def dev():
    return torch.device('cuda:0')


def name_of(dtype):
    return str(dtype).replace('torch.', '')


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def ceiling(dtype, n_grid, method):
    return DR.ceiling64(n_grid, method) if dtype == F64 else DR.ceiling32(n_grid, method)


@functools.lru_cache(maxsize=None)
def case(dim, batch, bias, dtype, method, t, step, last_only=False, seed=0):
    """(CPU module in `dtype`, y0, t, w, float64 reference gradients [y0, weight(, bias)], grid steps) - built once, shared, never modified."""
    torch.manual_seed(100 + seed)
    func = models.LinearODEFunc(dim, bias=bias, dtype=dtype)
    g = torch.Generator().manual_seed(200 + seed)
    if bias:
        with torch.no_grad():
            func.bias.copy_(0.5 * torch.randn(dim, generator=g, dtype=dtype))
    tt = torch.tensor(t, dtype=F64).to(dtype)
    y0 = torch.randn(batch, dim, generator=g, dtype=dtype)
    w = torch.randn(len(t), batch, dim, generator=g, dtype=dtype)
    if last_only:
        w[:-1] = 0.0
    f64 = copy.deepcopy(func).double()
    _, gy, gp = DGR.gradients(f64, tuple(f64.parameters()), y0.double(), tt.double(), method, step, w.double(), time_dtype=dtype)
    return func, y0, tt, w, gy + gp, DGR.n_grid_steps(tt, step, dtype)


def run(func_gpu, y0, t, w, method, step, **kw):
    for p in func_gpu.parameters():
        p.grad = None
    y = y0.to(dev()).clone().requires_grad_(True)
    odeint_discrete.last_backward_stats = {}
    sol = odeint_discrete(func_gpu, y, t, method=method, options={'step_size': step}, own_grid=True, **kw)
    assert sol.shape[0] == t.shape[0]
    (sol * w.to(dev())).sum().backward()
    return [y.grad] + [p.grad for p in func_gpu.parameters()], dict(odeint_discrete.last_backward_stats)


def kernel(stats, n_grid):
    assert stats['engine'] == KERNEL and stats['n_launches'] == 1 and stats['why'] == '' and stats['n_steps'] == n_grid, stats
    assert stats['own_grid']['n_grid_steps'] == n_grid and stats['own_grid']['recompute_launches'] == 0, stats
    assert stats['own_grid']['n_segments'] == 0 and stats['own_grid']['scratch_bytes'] > 0, stats


def compare(got, ref, ceil, what, dtype):
    assert len(got) == len(ref)
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a is not None and a.dtype == dtype, (what, i)
        err = DR.rel_max(a, b)
        worst = max(worst, err)
        print('%s %s tensor %d: %.3e (ceiling %.3e) ratio %.4f' % (what, name_of(dtype), i, err, ceil, err / ceil))
    assert worst <= ceil, '%s: max|got - ref| / max|ref| = %.3e above the ceiling %.3e' % (what, worst, ceil)
    return worst


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
@pytest.mark.parametrize('bias', (False, True), ids=('nobias', 'bias'))
@pytest.mark.parametrize('dim', (5, 16, 33, 128))
def test_every_instantiation_and_the_zero_padding(dim, bias, dtype):
    t, step = PAIRS['dyadic']
    func, y0, tt, w, ref, n_grid = case(dim, 21, bias, dtype, 'rk4', t, step)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, tt, w, 'rk4', step, linear='auto')
    kernel(stats, n_grid)
    compare(got, ref, ceiling(dtype, n_grid, 'rk4'), 'kernel dim %d bias=%s' % (dim, bias), dtype)


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
@pytest.mark.parametrize('pair', sorted(PAIRS))
@pytest.mark.parametrize('method', ('euler', 'midpoint', 'heun', 'rk4'))
def test_methods_on_the_three_grids(method, pair, dtype):
    t, step = PAIRS[pair]
    func, y0, tt, w, ref, n_grid = case(33, 21, True, dtype, method, t, step)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, tt, w, method, step, linear=True)
    kernel(stats, n_grid)
    assert stats['method'] == method
    compare(got, ref, ceiling(dtype, n_grid, method), 'kernel %s %s' % (method, pair), dtype)


def test_loss_on_the_last_output_only_and_sixteen_steps():
    """The ODEBlock shape: t = [0, 1], step_size 1 / 16, the loss on y(1)."""
    func, y0, tt, w, ref, n_grid = case(16, 40, True, F64, 'rk4', (0., 1.), 1 / 16, last_only=True)
    assert n_grid == 16
    got, stats = run(copy.deepcopy(func).to(dev()), y0, tt, w, 'rk4', 1 / 16, linear='auto')
    kernel(stats, 16)
    compare(got, ref, ceiling(F64, 16, 'rk4'), 'kernel t=[0,1] h=1/16', F64)


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
def test_batches_tiles_and_a_scratch_that_does_not_depend_on_the_batch(dtype):
    """Batch 1; batch 17: a ragged second tile; 16 x CUs - 3 rows: a ragged tile for every workgroup; 16 x CUs + 5 rows: more tiles than
    workgroups, so a workgroup walks a second tile over the scratch block of its first.  The scratch is grid x n_steps x 16 x D elements:
    a block per workgroup, whatever the batch."""
    t, step = PAIRS['clipped']
    esz = 8 if dtype == F64 else 4
    seen = {}
    for batch in (1, 17, 16 * cus() - 3, 16 * cus() + 5):
        func, y0, tt, w, ref, n_grid = case(16, batch, True, dtype, 'rk4', t, step)
        f = copy.deepcopy(func).to(dev())
        got, stats = run(f, y0, tt, w, 'rk4', step, linear='auto')
        kernel(stats, n_grid)
        compare(got, ref, ceiling(dtype, n_grid, 'rk4'), 'kernel batch %d' % batch, dtype)
        prof = stats['own_grid']                         # ('grid', 'scratch_bytes': the engine's own record of its last sweep)
        assert prof['scratch_bytes'] == prof['grid'] * n_grid * 16 * 16 * esz, prof
        seen[batch] = prof
    many = 16 * cus() + 5
    assert seen[many]['grid'] == min(cus(), 1024) and seen[many]['grid'] < (many + 15) // 16       # a workgroup owns a second tile
    assert seen[1]['grid'] == 1 and seen[17]['grid'] == 2
    assert seen[many]['scratch_bytes'] == seen[16 * cus() - 3]['scratch_bytes']                     # more rows, not more scratch
    assert seen[many]['scratch_bytes'] // seen[many]['grid'] == seen[17]['scratch_bytes'] // 2 == seen[1]['scratch_bytes']


def test_1024_grid_steps_are_taken_1025_are_refused_with_a_reason():
    func, y0, tt, w, ref, n_grid = case(16, 16, False, F64, 'rk4', (0., 1.), 1 / 1024, last_only=True)
    assert n_grid == 1024
    got, stats = run(copy.deepcopy(func).to(dev()), y0, tt, w, 'rk4', 1 / 1024, linear='auto')
    kernel(stats, 1024)
    compare(got, ref, ceiling(F64, 1024, 'rk4'), 'kernel 1024 steps', F64)
    func, y0, tt, w, ref, n_grid = case(16, 16, False, F64, 'euler', (0., 1.), 1 / 1025, last_only=True)
    assert n_grid == 1025
    f = copy.deepcopy(func).to(dev())
    got, stats = run(f, y0, tt, w, 'euler', 1 / 1025, linear='auto')
    assert stats['engine'] == 'fused linear sweep' and 'fused linear sweep (own grid): more than 1024 grid steps (1025)' in stats['why'], stats
    assert stats['n_steps'] == 1025 and stats['own_grid'] == {'n_grid_steps': 1025, 'n_segments': 2, 'recompute_launches': 3}, stats
    compare(got, ref, ceiling(F64, 1025, 'euler'), 'recompute 1025 steps', F64)


def test_more_than_1_gib_of_checkpoint_scratch_is_refused_and_the_recompute_takes_the_call():
    """dim 128 float64, 1024 grid steps: a workgroup's block is 1024 x 16 x 128 x 8 bytes = 16 MiB, and 66 tiles (batch 1043, the last one
    ragged) need 66 workgroups: 1056 MiB.  Create refuses before it allocates anything and 'auto' runs the recompute on the default-grid
    linear sweep.  (The smallest shape that reaches the bound; its float64 CPU reference is most of the test's time.)"""
    assert cus() >= 66
    func, y0, tt, w, ref, n_grid = case(128, 1043, False, F64, 'euler', (0., 1.), 1 / 1024, last_only=True)
    assert n_grid == 1024
    got, stats = run(copy.deepcopy(func).to(dev()), y0, tt, w, 'euler', 1 / 1024, linear='auto')
    assert stats['engine'] == 'fused linear sweep' and stats['n_steps'] == 1024, stats
    assert 'fused linear sweep (own grid): the fused engine could not be created' in stats['why'] and 'checkpoint scratch' in stats['why'], stats
    assert stats['own_grid']['n_segments'] >= 1 and stats['own_grid']['recompute_launches'] == 2 * stats['own_grid']['n_segments'] - 1, stats
    compare(got, ref, ceiling(F64, 1024, 'euler'), 'recompute after the scratch refusal', F64)
    with pytest.raises(ValueError, match='does not take this call'):
        # linear=True raises only where the default-grid linear sweep refuses as well: 1025 steps cut in two segments do not, a tuple state does
        odeint_discrete(copy.deepcopy(func).to(dev()), (y0.to(dev()), y0.to(dev())), tt, method='euler',
                        options={'step_size': 1 / 1024}, own_grid=True, linear=True)


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
def test_two_backward_calls_give_identical_bits(dtype):
    t, step = PAIRS['dyadic']
    func, y0, tt, w, ref, n_grid = case(33, 16 * cus() + 5, True, dtype, 'rk4', t, step)
    f = copy.deepcopy(func).to(dev())
    a, stats = run(f, y0, tt, w, 'rk4', step, linear='auto')
    kernel(stats, n_grid)
    b, _ = run(f, y0, tt, w, 'rk4', step, linear='auto')
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    compare(a, ref, ceiling(dtype, n_grid, 'rk4'), 'kernel two calls', dtype)


def test_the_callable_forms_the_module_and_an_in_place_optimizer_step():
    t, step = PAIRS['clipped']
    func, y0, tt, w, ref, n_grid = case(16, 21, True, F64, 'heun', t, step)
    W = func.weight.detach().to(dev()).clone().requires_grad_(True)
    b = func.bias.detach().to(dev()).clone().requires_grad_(True)
    lin = torch.nn.Linear(16, 16).double().to(dev())
    with torch.no_grad():
        lin.weight.copy_(W.t())
        lin.bias.copy_(b)

    class Lin(torch.nn.Module):
        def __init__(self):
            super(Lin, self).__init__()
            self.lin = lin

        def forward(self, t_, y):
            return self.lin(y)
    nobias = case(16, 21, False, F64, 'heun', t, step)
    W2 = nobias[0].weight.detach().to(dev()).clone().requires_grad_(True)
    forms = (('y @ W + b', (lambda t_, y: y @ W + b), (W, b), (y0, w, ref), lambda g: g),
             ('y @ W', (lambda t_, y: y @ W2), (W2,), (nobias[1], nobias[3], nobias[4]), lambda g: g),
             ('nn.Linear', Lin(), (lin.weight, lin.bias), (y0, w, ref), lambda g: [g[0], g[1].t(), g[2]]))
    for what, f, params, (y0_, w_, ref_), fix in forms:
        for p in params:
            p.grad = None
        y = y0_.to(dev()).clone().requires_grad_(True)
        (odeint_discrete(f, y, tt, method='heun', options={'step_size': step}, own_grid=True, linear=True) * w_.to(dev())).sum().backward()
        kernel(dict(odeint_discrete.last_backward_stats), n_grid)
        compare(fix([y.grad] + [p.grad for p in params]), ref_, ceiling(F64, n_grid, 'heun'), 'kernel ' + what, F64)
    # the module, twice, with an in-place step between: the second backward reads the new weights
    f = copy.deepcopy(func).to(dev())
    got, stats = run(f, y0, tt, w, 'heun', step, linear='auto')
    kernel(stats, n_grid)
    compare(got, ref, ceiling(F64, n_grid, 'heun'), 'kernel module', F64)
    with torch.no_grad():
        for p in f.parameters():
            p.mul_(0.5)
    moved = copy.deepcopy(f).cpu()
    _, gy, gp = DGR.gradients(moved, tuple(moved.parameters()), y0, tt, 'heun', step, w)
    got2, stats = run(f, y0, tt, w, 'heun', step, linear='auto')
    kernel(stats, n_grid)
    compare(got2, gy + gp, ceiling(F64, n_grid, 'heun'), 'kernel after an in-place step', F64)
    assert not torch.equal(got[1], got2[1])


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
def test_grid_kernel_off_takes_the_recompute_and_the_default_grid_linear_sweep(dtype, monkeypatch):
    t, step = PAIRS['dyadic']
    func, y0, tt, w, ref, n_grid = case(33, 21, True, dtype, 'rk4', t, step)
    monkeypatch.setattr(discrete, 'GRID_KERNEL', False)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, tt, w, 'rk4', step, linear='auto')
    assert stats['engine'] == 'fused linear sweep' and stats['n_launches'] == 1 and stats['n_steps'] == n_grid, stats
    assert stats['own_grid'] == {'n_grid_steps': n_grid, 'n_segments': 1, 'recompute_launches': 1}, stats
    assert 'discrete.GRID_KERNEL is False' in stats['why']
    compare(got, ref, ceiling(dtype, n_grid, 'rk4'), 'recompute + linear sweep', dtype)


def test_three_segments_on_the_default_grid_linear_sweep(monkeypatch):
    t, step = (0., 0.375, 0.4, 0.45, 1.0), 0.125
    func, y0, tt, w, ref, n_grid = case(16, 21, True, F64, 'rk4', t, step)
    assert n_grid == 8
    monkeypatch.setattr(discrete, 'GRID_KERNEL', False)
    monkeypatch.setattr(discrete, 'GRID_BYTES', 8 * y0.numel() * 8)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, tt, w, 'rk4', step, linear='auto')
    assert stats['engine'] == 'fused linear sweep' and stats['n_launches'] == 3, stats
    assert stats['own_grid'] == {'n_grid_steps': 8, 'n_segments': 3, 'recompute_launches': 5}, stats
    compare(got, ref, ceiling(F64, 8, 'rk4'), 'recompute in 3 segments', F64)


def test_recompute_route_on_the_fused_mlp_sweep():
    torch.manual_seed(31)
    func = models.ODEFunc(4, 8, non_linearity='tanh')
    g = torch.Generator().manual_seed(32)
    y0 = torch.randn(40, 4, generator=g)
    t, step = (0., 0.3, 1.0), 0.25
    tt = torch.tensor(t)
    w = torch.randn(3, 40, 4, generator=g)
    f64 = copy.deepcopy(func).double()
    _, gy, gp = DGR.gradients(f64, tuple(f64.parameters()), y0.double(), tt.double(), 'rk4', step, w.double(), time_dtype=F32)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, tt, w, 'rk4', step)
    assert stats['engine'] == 'fused mlp sweep' and stats['n_launches'] == 1 and stats['n_steps'] == 4, stats
    assert stats['own_grid'] == {'n_grid_steps': 4, 'n_segments': 1, 'recompute_launches': 1}, stats
    compare(got, gy + gp, ceiling(F32, 4, 'rk4'), 'recompute + mlp sweep', F32)


def test_recompute_route_on_the_fused_row_local_sweep():
    f, params, y0 = DC.SYSTEMS['tanh8'](str(dev()), F64)
    fc, pc, y0c = DC.SYSTEMS['tanh8']('cpu', F64)
    t, step = PAIRS['clipped']
    tt = torch.tensor(t, dtype=F64)
    w = torch.randn((len(t),) + tuple(y0c.shape), generator=torch.Generator().manual_seed(33), dtype=F64)
    _, gy, gp = DGR.gradients(fc, pc, y0c, tt, 'midpoint', step, w)
    y = y0.clone().requires_grad_(True)
    sol = odeint_discrete(f, y, tt, method='midpoint', options={'step_size': step}, own_grid=True, lower='auto')
    got = torch.autograd.grad((sol * w.to(dev())).sum(), (y,) + tuple(params))
    stats = odeint_discrete.last_backward_stats
    assert stats['engine'] == 'fused row-local sweep' and stats['n_launches'] == 1 and stats['n_steps'] == 4, stats
    assert stats['own_grid'] == {'n_grid_steps': 4, 'n_segments': 1, 'recompute_launches': 1}, stats
    compare(list(got), gy + gp, ceiling(F64, 4, 'midpoint'), 'recompute + row-local sweep', F64)


def test_recompute_route_on_the_generic_sweep_with_a_tuple_state():
    torch.manual_seed(34)
    net = torch.nn.Linear(4, 3).double()

    def make(n):
        def func(t_, y):
            a, b = y
            return torch.tanh(n(b)) * (1.0 + t_), torch.sin(a) @ n.weight
        return func
    g = torch.Generator().manual_seed(35)
    y0 = (torch.randn(9, 3, generator=g, dtype=F64), torch.randn(9, 4, generator=g, dtype=F64))
    t, step = PAIRS['dyadic']
    tt = torch.tensor(t, dtype=F64)
    w = tuple(torch.randn((len(t),) + tuple(y.shape), generator=g, dtype=F64) for y in y0)
    _, gy, gp = DGR.gradients(make(net), tuple(net.parameters()), y0, tt, 'heun', step, w)
    net_gpu = copy.deepcopy(net).to(dev())
    ys = tuple(y.to(dev()).clone().requires_grad_(True) for y in y0)
    sol = odeint_discrete(make(net_gpu), ys, tt, method='heun', options={'step_size': step}, own_grid=True)
    got = torch.autograd.grad(sum((w_.to(dev()) * s).sum() for w_, s in zip(w, sol)), ys + tuple(net_gpu.parameters()))
    stats = odeint_discrete.last_backward_stats
    assert stats['engine'] == 'generic sweep' and stats['n_steps'] == 4, stats
    assert stats['own_grid'] == {'n_grid_steps': 4, 'n_segments': 1, 'recompute_launches': 1}, stats
    compare(list(got), gy + gp, ceiling(F64, 4, 'heun'), 'recompute + generic sweep (tuple)', F64)
