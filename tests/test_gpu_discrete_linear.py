"""GPU tests of the fused linear sweep (csrc/mi_ode_discrete_linear.h, odeint_discrete(linear='auto')): the gradients of
sum_n w_n . y_n, random w at every grid point, against autograd through the float64 CPU restatement of the same discrete map
(tests/discrete_restatement.py).

Metric, per gradient tensor: DR.rel_max = max|got - ref| / max|ref|.  Ceilings: DR.ceiling64(n_steps, method) for float64 and
DR.ceiling32(n_steps, method) for float32, the ones of tests/test_gpu_discrete.py.  Every fused case asserts the engine's name and that the
whole backward was one launch.  Each comparison prints its figure and its share of the ceiling ("ratio"); observed values:
profiles/discrete_linear_gpu_tests.txt.
"""
import copy
import functools

import pytest
import torch

from tfdiffeq_amd import discrete, models, odeint_discrete
from tests import discrete_restatement as DR

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
# (dim, batch, bias): every kernel width (16 / 32 / 64 / 128), padded columns (5, 24, 100), dim 5 - the smallest the tracer calls linear;
# batch 7: less than a tile; 200: a ragged last tile; 4136 rows at dim 16: 259 tiles, more than the 256 workgroups, so a workgroup owns
# several; 7 and 48: fewer tiles than the grid (one workgroup per 1024 entries of the fold), workgroups without tiles
GEOMETRY = ((5, 7, True), (16, 4136, False), (24, 200, True), (64, 48, False), (64, 200, True), (100, 200, True), (128, 48, True), (128, 7, False))
GRIDS = (('euler', 2), ('midpoint', 5), ('heun', 5), ('rk4', 5), ('rk4', 21))


def dev():
    return torch.device('cuda:0')


def name_of(dtype):
    return str(dtype).replace('torch.', '')


def ceiling(dtype, n, method):
    return DR.ceiling64(n - 1, method) if dtype == F64 else DR.ceiling32(n - 1, method)


@functools.lru_cache(maxsize=None)
def case(dim, batch, bias, dtype, method, n, grid='uniform', seed=0):
    """(CPU module in `dtype`, y0, t, w, float64 reference gradients [y0, weight(, bias)]) - built once, shared, never modified."""
    torch.manual_seed(100 + seed)
    func = models.LinearODEFunc(dim, bias=bias, dtype=dtype)
    g = torch.Generator().manual_seed(200 + seed)
    if bias:
        with torch.no_grad():
            func.bias.copy_(0.5 * torch.randn(dim, generator=g, dtype=dtype))
    t = torch.linspace(0., 1., n, dtype=dtype)
    if grid == 'nonuniform':
        t = t ** 1.7
    elif grid == 'decreasing':
        t = torch.flip(t, (0,)).contiguous()
    y0 = torch.randn(batch, dim, generator=g, dtype=dtype)
    w = torch.randn(n, batch, dim, generator=g, dtype=dtype)
    return func, y0, t, w, reference64(func, y0, t, w, method)


def reference64(func, y0, t, w, method):
    f64 = copy.deepcopy(func).double()
    _, gy, gp = DR.gradients(f64, tuple(f64.parameters()), y0.double(), t.double(), method, w.double())
    return gy + gp


def run(func_gpu, y0, t, w, method, **kw):
    for p in func_gpu.parameters():
        p.grad = None
    y = y0.to(dev()).clone().requires_grad_(True)
    odeint_discrete.last_backward_stats = {}
    sol = odeint_discrete(func_gpu, y, t, method=method, **kw)
    (sol * w.to(dev())).sum().backward()
    return [y.grad] + [p.grad for p in func_gpu.parameters()], dict(odeint_discrete.last_backward_stats)


def fused(stats):
    assert stats['engine'] == 'fused linear sweep' and stats['n_launches'] == 1 and stats['why'] == '', stats


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
@pytest.mark.parametrize('dim,batch,bias', GEOMETRY)
def test_geometry(dim, batch, bias, dtype):
    func, y0, t, w, ref = case(dim, batch, bias, dtype, 'rk4', 5)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, t, w, 'rk4', linear='auto')
    fused(stats)
    compare(got, ref, ceiling(dtype, 5, 'rk4'), 'geometry %dx%d bias=%s' % (batch, dim, bias), dtype)


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
@pytest.mark.parametrize('method,n', GRIDS)
def test_methods(method, n, dtype):
    func, y0, t, w, ref = case(24, 200, True, dtype, method, n)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, t, w, method, linear='auto')
    fused(stats)
    assert stats['n_steps'] == n - 1 and stats['method'] == method
    compare(got, ref, ceiling(dtype, n, method), '%s N=%d' % (method, n), dtype)


def test_huen_is_heun():
    func, y0, t, w, ref = case(24, 200, True, F64, 'heun', 5)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, t, w, 'huen', linear=True)
    fused(stats)
    compare(got, ref, ceiling(F64, 5, 'heun'), 'huen N=5', F64)


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
@pytest.mark.parametrize('grid', ('nonuniform', 'decreasing'))
def test_grids(grid, dtype):
    func, y0, t, w, ref = case(24, 200, True, dtype, 'rk4', 5, grid)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, t, w, 'rk4', linear='auto')
    fused(stats)
    compare(got, ref, ceiling(dtype, 5, 'rk4'), 'rk4 N=5 %s grid' % grid, dtype)


def test_1025_points_are_accepted():
    func, y0, t, w, ref = case(16, 16, True, F64, 'rk4', 1025)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, t, w, 'rk4', linear='auto')
    fused(stats)
    assert stats['n_steps'] == 1024
    compare(got, ref, ceiling(F64, 1025, 'rk4'), 'rk4 N=1025', F64)


def test_1026_points_take_the_generic_sweep_and_say_why():
    torch.manual_seed(5)
    func = models.LinearODEFunc(16, bias=False, dtype=F64).to(dev())
    y0 = torch.randn(16, 16, dtype=F64, generator=torch.Generator().manual_seed(6))
    t = torch.linspace(0., 1., 1026, dtype=F64)
    y = y0.to(dev()).requires_grad_(True)
    sol = odeint_discrete(func, y, t, method='euler', linear='auto')
    sol[-1].sum().backward()
    stats = odeint_discrete.last_backward_stats
    assert stats['engine'] == 'generic sweep' and 'fused linear sweep: more than 1024 steps (1025)' in stats['why'], stats
    assert bool(torch.isfinite(y.grad).all()) and bool(torch.isfinite(func.weight.grad).all())
    with pytest.raises(ValueError, match='more than 1024 steps'):
        odeint_discrete(func, y0.to(dev()).requires_grad_(True), t, method='euler', linear=True)


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
def test_loss_on_the_last_point_only(dtype):
    """Zero output gradients at every grid point but the last: grad_y0 is the product of the transposed steps alone."""
    func, y0, t, w, _ = case(24, 200, True, dtype, 'rk4', 5)
    w_last = torch.zeros_like(w)
    w_last[-1] = w[-1]
    ref = reference64(func, y0, t, w_last, 'rk4')
    got, stats = run(copy.deepcopy(func).to(dev()), y0, t, w_last, 'rk4', linear='auto')
    fused(stats)
    compare(got, ref, ceiling(dtype, 5, 'rk4'), 'loss on the last point', dtype)


class LinModule(torch.nn.Module):
    """torch.nn.Linear(d, d) as a right-hand side: the matrix is [out, in]."""

    def __init__(self, d, dtype):
        super(LinModule, self).__init__()
        self.lin = torch.nn.Linear(d, d).to(dtype)

    def forward(self, t, y):
        return self.lin(y)


def _callable_case(form, dtype, d=16, batch=48):
    g = torch.Generator().manual_seed(31)
    W = (-0.5 * torch.eye(d, dtype=dtype) + 0.3 * torch.randn(d, d, generator=g, dtype=dtype) / d ** 0.5)
    b = 0.5 * torch.randn(d, generator=g, dtype=dtype)
    y0 = torch.randn(batch, d, generator=g, dtype=dtype)
    t = torch.linspace(0., 1., 5, dtype=dtype)
    w = torch.randn(5, batch, d, generator=g, dtype=dtype)

    def make(device, dt):
        Wd = W.detach().clone().to(device=device, dtype=dt).requires_grad_(True)        # (leaves of their own: .to() alone may return W itself)
        bd = b.detach().clone().to(device=device, dtype=dt).requires_grad_(True)
        if form == 'matmul':
            return (lambda t_, y: y @ Wd), (Wd,)
        if form == 'matmul_bias':
            return (lambda t_, y: y @ Wd + bd), (Wd, bd)
        if form == 'transposed':
            return (lambda t_, y: y @ Wd.t()), (Wd,)
        mod = LinModule(d, dt)
        with torch.no_grad():
            mod.lin.weight.copy_(W.to(dt))
            mod.lin.bias.copy_(b.to(dt))
        mod = mod.to(device)
        return mod, tuple(mod.parameters())
    f64, p64 = make('cpu', F64)
    _, gy, gp = DR.gradients(f64, p64, y0.double(), t.double(), 'rk4', w.double())
    return make, y0, t, w, gy + gp


@pytest.mark.parametrize('dtype', (F64, F32), ids=name_of)
@pytest.mark.parametrize('form', ('matmul', 'matmul_bias', 'nn_linear'))
def test_callable_forms(form, dtype):
    """`y @ W`, `y @ W + b` and torch.nn.Linear(d, d) - whose [out, in] matrix gets its gradient back in that layout - reach the kernel."""
    make, y0, t, w, ref = _callable_case(form, dtype)
    f, params = make(dev(), dtype)
    y = y0.to(dev()).requires_grad_(True)
    odeint_discrete.last_backward_stats = {}
    got = torch.autograd.grad((odeint_discrete(f, y, t, method='rk4', linear='auto') * w.to(dev())).sum(), (y,) + tuple(params))
    fused(dict(odeint_discrete.last_backward_stats))
    for a, p in zip(got[1:], params):
        assert a.shape == p.shape
    compare(list(got), ref, ceiling(dtype, 5, 'rk4'), 'callable %s' % form, dtype)


def test_a_derived_matrix_is_refused_and_the_generic_sweep_is_right():
    make, y0, t, w, ref = _callable_case('transposed', F64)
    f, params = make(dev(), F64)
    y = y0.to(dev()).requires_grad_(True)
    got = torch.autograd.grad((odeint_discrete(f, y, t, method='rk4', linear='auto') * w.to(dev())).sum(), (y,) + tuple(params))
    stats = odeint_discrete.last_backward_stats
    assert stats['engine'] == 'generic sweep' and 'fused linear sweep: a derived (non-leaf)' in stats['why'], stats
    compare(list(got), ref, ceiling(F64, 5, 'rk4'), 'derived matrix, generic sweep', F64)
    with pytest.raises(ValueError, match='derived'):
        odeint_discrete(f, y0.to(dev()).requires_grad_(True), t, method='rk4', linear=True)


def test_module_route_through_odeblock(monkeypatch):
    monkeypatch.setattr(discrete, 'LINEAR', 'auto')
    func, y0, _, w, _ = case(24, 200, True, F64, 'rk4', 5)
    t = torch.tensor([0., 1.], dtype=F64)                    # the block's integration interval; it returns the state at 1
    w2 = torch.stack([torch.zeros_like(w[0]), w[1]])
    ref = reference64(func, y0, t, w2, 'rk4')
    block = models.ODEBlock(copy.deepcopy(func), solver='rk4', gradient='discrete').to(dev())
    x = y0.to(dev()).requires_grad_(True)
    odeint_discrete.last_backward_stats = {}
    (block(x) * w[1].to(dev())).sum().backward()
    fused(dict(odeint_discrete.last_backward_stats))
    compare([x.grad] + [p.grad for p in block.odefunc.parameters()], ref, ceiling(F64, 2, 'rk4'), 'ODEBlock', F64)


def test_two_calls_are_bit_identical():
    func, y0, t, w, _ = case(100, 200, True, F64, 'rk4', 5)
    fg = copy.deepcopy(func).to(dev())
    a, sa = run(fg, y0, t, w, 'rk4', linear='auto')
    a = [x.clone() for x in a]
    b, sb = run(fg, y0, t, w, 'rk4', linear='auto')
    fused(sa)
    fused(sb)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_an_in_place_step_between_two_calls_is_seen():
    func, y0, t, w, ref = case(24, 200, True, F64, 'rk4', 5)
    fg = copy.deepcopy(func).to(dev())
    got, stats = run(fg, y0, t, w, 'rk4', linear='auto')
    fused(stats)
    compare(got, ref, ceiling(F64, 5, 'rk4'), 'before the step', F64)
    stepped = copy.deepcopy(func)
    with torch.no_grad():                                    # one SGD step with the reference's gradients, on both copies
        for p_gpu, p_cpu, g in zip(fg.parameters(), stepped.parameters(), ref[1:]):
            p_gpu.sub_(0.05 * g.to(dev()) / g.abs().max())
            p_cpu.sub_(0.05 * g / g.abs().max())
    ref2 = reference64(stepped, y0, t, w, 'rk4')
    assert DR.rel_max(ref2[1], ref[1]) > 1e-3                # the step moves the gradient far beyond the ceiling
    got2, stats2 = run(fg, y0, t, w, 'rk4', linear='auto')
    fused(stats2)
    compare(got2, ref2, ceiling(F64, 5, 'rk4'), 'after the step', F64)


def test_two_modules_share_the_cached_engine_and_keep_their_own_gradients():
    fa, y0, t, w, ref_a = case(24, 200, True, F64, 'rk4', 5)
    fb, y0b, _, wb, ref_b = case(24, 200, True, F64, 'rk4', 5, 'uniform', 1)
    discrete.clear_engines()
    ga, gb = copy.deepcopy(fa).to(dev()), copy.deepcopy(fb).to(dev())
    ya, yb = y0.to(dev()).requires_grad_(True), y0b.to(dev()).requires_grad_(True)
    sol_a = odeint_discrete(ga, ya, t, method='rk4', linear='auto')
    sol_b = odeint_discrete(gb, yb, t, method='rk4', linear='auto')
    assert len(discrete._LINEAR_ENGINES) == 1
    (sol_a * w.to(dev())).sum().backward()
    fused(dict(odeint_discrete.last_backward_stats))
    (sol_b * wb.to(dev())).sum().backward()
    fused(dict(odeint_discrete.last_backward_stats))
    compare([ya.grad] + [p.grad for p in ga.parameters()], ref_a, ceiling(F64, 5, 'rk4'), 'module A', F64)
    compare([yb.grad] + [p.grad for p in gb.parameters()], ref_b, ceiling(F64, 5, 'rk4'), 'module B', F64)


def test_the_default_is_still_the_generic_sweep():
    assert discrete.LINEAR is False
    func, y0, t, w, ref = case(24, 200, True, F64, 'rk4', 5)
    got, stats = run(copy.deepcopy(func).to(dev()), y0, t, w, 'rk4')
    assert stats['engine'] == 'generic sweep' and 'fused linear sweep' not in stats['why'], stats
    compare(got, ref, ceiling(F64, 5, 'rk4'), 'default route', F64)
