"""GPU tests of the fused hypersolver gradient (options={'grad': 'auto' | True}; csrc/mi_ode_hyper_grad.h): every case of
tests/hyper_grad_cases.py against the float64 CPU eager loop under autograd at the bounds stated there, the engine contract (stats, the
forward bit-equal to the no-grad call, bit-identical reruns, saved parameters, interleaved solvers, streams) and the calls outside the
box.  Shapes are tiny: T is 2, 3 or 9, D is 2 or 3."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import hyper_cases as EC
from tests import hyper_grad_cases as GC
from tests import hyper_restatement as HR
from tfdiffeq_amd import _native as N
from tfdiffeq_amd import hyper_solvers as H
from tfdiffeq_amd import rhs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PACKED = ('packed_128', 'packed_notebook', 'f32_packed_128')


@pytest.fixture
def grad_grid():
    """Sets hyper_solvers.GRAD_GRID for one test and puts it back."""
    old = H.GRAD_GRID

    def set_(v):
        H.GRAD_GRID = v
    yield set_
    H.GRAD_GRID = old


def _run(case, options=None, **kw):
    return GC.run(case, GC.torch_dtype(case), device=DEV, options={'grad': True, 'lower': True} if options is None else options, **kw)


@pytest.mark.parametrize('case', GC.CASES, ids=lambda c: c.name)
def test_fused_gradients_match_the_cpu_oracle(case, grad_grid):
    """What each case is there to break is said next to it in tests/hyper_grad_cases.py: rows per tile and tiles per workgroup, the fold,
    widths and padding, layers and activations, both weight paths, methods, grids, systems, cotangents, leaves."""
    grad_grid(case.grad_grid)
    ref_out, ref, _ = GC.oracle(case)
    out, got, solver = _run(case)
    st, bst = solver.last_stats, solver.last_backward_stats
    assert st['engine'] == 'fused' and st['grad'] == 'fused' and bst['engine'] == 'fused', (st, bst)
    assert bst['n_launches'] == (2 if case.name in PACKED else 1), bst
    work = case.B * (len(GC.GRIDS[case.grid]) if case.op == 'gresid' else 1)
    tiles = (work + 15) // 16
    assert bst['grid'] == min(tiles, case.grad_grid or H.GRAD_DEFAULT_GRID), bst
    if case.name == 'default_grid':
        assert bst['grid'] == H.GRAD_DEFAULT_GRID and tiles == H.GRAD_DEFAULT_GRID + 1
    if case.name == 'b37_grid2':
        assert bst['grid'] == 2 and tiles == 3                 # two trips for workgroup 0, one for workgroup 1, a ragged last tile
    dev = GC.deviations(got, ref)
    bound = GC.bound_of(case)
    print(case.name, 'bound %.3e' % bound, ' '.join('%s %.3e' % kv for kv in sorted(dev.items())))
    assert dev and max(dev.values()) <= bound, (case.name, dev, bound)
    fwd = float((out.cpu().double() - ref_out).abs().max() / ref_out.abs().max())
    assert fwd <= (1e-11 if case.dtype == 'float64' else 1e-4)
    if case.cot == 'row0':                                     # the parameter gradients are exactly zero and grad y0 is G[0]
        assert all(g is None or float(g.abs().max()) == 0.0 for g in got['params'])
        assert torch.equal(got['y0'].cpu(), torch.tensor(GC.cotangent_of(case)[0], dtype=GC.torch_dtype(case)))
    if case.leaves != 'all':                                   # None for what is not a leaf
        for name, is_leaf in got['leaf'].items():
            g = got['y0'] if name == 'y0' else got['params'][int(name[1:])]
            assert (g is not None) == is_leaf, (name, is_leaf)


def _setup(name, options, dtype=None, method=None):
    case = GC.BY_NAME[name]
    dtype = dtype or GC.torch_dtype(case)
    g = GC.make_g(case, dtype=dtype, device=DEV)
    s = GC.solver_of(case, GC.make_f(case), g, options) if method is None else method(GC.make_f(case), g, options=options)
    t = torch.tensor(GC.grid_of(case), dtype=dtype, device=DEV)
    y = torch.tensor(GC.y0_of(case), dtype=dtype, device=DEV)
    G = torch.tensor(GC.cotangent_of(case), dtype=dtype, device=DEV)
    return case, s, g, t, y, G


def test_forward_is_bit_equal_to_the_no_grad_call_and_stats_are_as_specified():
    for name in ('b37', 'packed_notebook', 'f32_heun', 'gresid'):
        case, s, g, t, y, G = _setup(name, {'grad': 'auto'})
        if case.op == 'gresid':
            y = torch.tensor(GC.base_of(case), dtype=y.dtype, device=DEV)
        out = GC.call(case, s, t, y)
        assert out.requires_grad and s.last_stats['engine'] == 'fused' and s.last_stats['grad'] == 'fused' and s.last_backward_stats == {}
        with torch.no_grad():
            plain = GC.call(case, s, t, y)
        assert 'grad' not in s.last_stats and s.last_stats['engine'] == 'fused' and not plain.requires_grad
        assert torch.equal(out.detach(), plain)
        (out * G).sum().backward()
        assert set(s.last_backward_stats) >= {'engine', 'n_launches', 'grid', 'why'} and s.last_backward_stats['n_launches'] in (1, 2)
    # nothing requires grad: the existing no-grad path, whatever the option
    case, s, g, t, y, G = _setup('b37', {'grad': True})
    g.requires_grad_(False)
    out = s.trajectory(t, y)
    assert not out.requires_grad and s.last_stats['engine'] == 'fused' and 'grad' not in s.last_stats


@pytest.mark.parametrize('name,grid', [('b37', 0), ('b37', 2), ('f32_grid2', 2), ('packed_notebook', 0), ('gresid_grid2', 2)])
def test_two_runs_agree_in_every_bit(name, grid, grad_grid):
    grad_grid(grid)
    case = GC.BY_NAME[name]
    _, a, _ = _run(case)
    _, b, _ = _run(case)
    for x, y in zip([a['y0']] + a['params'], [b['y0']] + b['params']):
        assert (x is None and y is None) or torch.equal(x, y)


def test_grad_accumulates_over_two_backward_calls():
    case, s, g, t, y, G = _setup('b17', {'grad': True})
    y.requires_grad_(True)
    (s.trajectory(t, y) * G).sum().backward()
    once = [y.grad.clone()] + [p.grad.clone() for p in g.parameters()]
    (s.trajectory(t, y) * G).sum().backward()
    for a, b in zip(once, [y.grad] + [p.grad for p in g.parameters()]):
        assert torch.equal(b, a + a)


def test_optimizer_step_is_seen_and_in_place_change_before_backward_raises():
    case, s, g, t, y, G = _setup('b17', {'grad': True})
    opt = torch.optim.SGD(g.parameters(), lr=0.1)
    out1 = s.trajectory(t, y)
    (out1 * G).sum().backward()
    first = [p.grad.clone() for p in g.parameters()]
    opt.step()
    opt.zero_grad()
    out2 = s.trajectory(t, y)
    assert not torch.equal(out1.detach(), out2.detach())     # the second forward read the new weights
    with torch.no_grad():
        assert torch.equal(out2.detach(), s.trajectory(t, y))
    (out2 * G).sum().backward()
    assert any(not torch.equal(a, p.grad) for a, p in zip(first, g.parameters()))
    out3 = s.trajectory(t, y)
    opt.step()                                                 # in place, between forward and backward
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        (out3 * G).sum().backward()


def test_two_solvers_interleaved_keep_their_own_gradients():
    ca, sa, ga, ta, ya, Ga = _setup('b17', {'grad': True})
    cb, sb, gb, tb, yb, Gb = _setup('w64', {'grad': True})
    oa = sa.trajectory(ta, ya)
    ob = sb.trajectory(tb, yb)
    (oa * Ga).sum().backward()
    (ob * Gb).sum().backward()
    for case, g in ((ca, ga), (cb, gb)):
        _, ref, _ = GC.oracle(case)
        got = {'y0': None, 'params': [p.grad for p in g.parameters()]}
        ref = {'y0': None, 'params': ref['params']}
        assert max(GC.deviations(got, ref).values()) <= GC.F64_BOUND


def test_backward_on_a_non_default_stream():
    case, s, g, t, y, G = _setup('b37', {'grad': True})
    _, ref, _ = GC.oracle(case)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        y.requires_grad_(True)
        (s.trajectory(t, y) * G).sum().backward()
    side.synchronize()
    got = {'y0': y.grad, 'params': [p.grad for p in g.parameters()]}
    assert max(GC.deviations(got, ref).values()) <= GC.F64_BOUND


# ---- outside the box ----------------------------------------------------------------------------------------------------------------------
class _Wrapped(nn.Module):
    def __init__(self, net):
        super(_Wrapped, self).__init__()
        self.net = net

    def forward(self, x):
        return self.net(x)


class _TrainableF(nn.Module):
    def __init__(self):
        super(_TrainableF, self).__init__()
        self.a = nn.Parameter(torch.tensor(0.7, dtype=torch.float64))

    def forward(self, t, y):
        return torch.stack([y[..., 1], -self.a * y[..., 0]], dim=-1)


def _net(widths):
    mods = []
    for i in range(len(widths) - 1):
        mods += [nn.Linear(widths[i], widths[i + 1])] + ([nn.Tanh()] if i < len(widths) - 2 else [])
    return nn.Sequential(*mods).double()


OUTSIDE = {
    'trainable_f': (lambda: _TrainableF(), lambda: _net([5, 17, 2]), 2, False, 'trainable'),
    'custom_rowlocal': (lambda: EC.ring(2), lambda: _net([5, 17, 2]), 2, False, 'CustomRowLocal'),
    't_span_requires_grad': (lambda: rhs.LotkaVolterra(), lambda: _net([5, 17, 2]), 2, True, 't_span requires grad'),
    'beyond_the_size_limit': (lambda: rhs.LotkaVolterra(), lambda: _net([5] + [128] * 5 + [2]), 2, False, 'size limit'),
    'not_sequential': (lambda: rhs.LotkaVolterra(), lambda: _Wrapped(_net([5, 17, 2])), 2, False, 'not an nn.Sequential'),
}


@pytest.mark.parametrize('name', sorted(OUTSIDE))
def test_outside_the_box_auto_trains_on_eager_and_true_raises(name):
    mk_f, mk_g, D, t_grad, word = OUTSIDE[name]
    torch.manual_seed(3)
    f_cpu, g_cpu = mk_f(), mk_g()
    y0 = torch.tensor([1., 0.5]) .double() + 0.2 * torch.randn(5, D, dtype=torch.float64)
    G = torch.randn(3, 5, D, dtype=torch.float64)
    t = torch.tensor(GC.MAIN[:3], dtype=torch.float64)

    def grads(dev, options, eager=False):
        import copy
        f, g = copy.deepcopy(f_cpu), copy.deepcopy(g_cpu).to(dev)
        if isinstance(f, nn.Module):
            f = f.to(dev)
        s = H.HyperHeun(f, g, options=options)
        tt = t.detach().clone().to(dev).requires_grad_(t_grad)
        y = y0.detach().clone().to(dev).requires_grad_(True)
        out = s._eager(N.HYPER_TRAJECTORY, tt, y) if eager else s.trajectory(tt, y)
        (out * G.to(dev)).sum().backward()
        ps = list(g.parameters()) + (list(f.parameters()) if isinstance(f, nn.Module) else []) + ([tt] if t_grad else [])
        return s, [y.grad.cpu()] + [p.grad.cpu() for p in ps]

    _, ref = grads('cpu', None, eager=True)
    s, got = grads(DEV, {'grad': 'auto'})
    assert s.last_stats['engine'] == 'eager' and word in s.last_stats['why'] and 'grad' not in s.last_stats, s.last_stats
    assert s.last_backward_stats == {}
    for a, b in zip(got, ref):
        assert float((a - b).abs().max()) <= GC.F64_BOUND * float(b.abs().max())
    with pytest.raises(ValueError, match=word):
        grads(DEV, {'grad': True})
    s, _ = grads(DEV, None)                                    # the option unset: the eager engine, as before
    assert s.last_stats['engine'] == 'eager' and 'autograd' in s.last_stats['why']


def test_base_trajectory_that_requires_grad_is_outside_the_box():
    case = GC.BY_NAME['gresid']
    g = GC.make_g(case, device=DEV)
    s = H.HyperEuler(GC.make_f(case), g, options={'grad': 'auto'})
    t = torch.tensor(GC.grid_of(case), device=DEV)
    base = torch.tensor(GC.base_of(case), device=DEV, requires_grad=True)
    s._hypersolver_residuals(t, base).sum().backward()
    assert s.last_stats['engine'] == 'eager' and 'base trajectory requires grad' in s.last_stats['why'] and base.grad is not None
    with pytest.raises(ValueError, match='base trajectory requires grad'):
        H.HyperEuler(GC.make_f(case), g, options={'grad': True})._hypersolver_residuals(t, base)


def test_module_default_switches_the_option():
    case, s, g, t, y, G = _setup('b17', None)
    old = H.FUSED_GRAD
    try:
        H.FUSED_GRAD = 'auto'
        (s.trajectory(t, y) * G).sum().backward()
        assert s.last_stats['engine'] == 'fused' and s.last_backward_stats['engine'] == 'fused'
    finally:
        H.FUSED_GRAD = old
    s.trajectory(t, y)
    assert s.last_stats['engine'] == 'eager'


# ---- against the eager engine on the GPU: the notebook shape ----------------------------------------------------------------------------
def test_notebook_shape_against_the_eager_engine_on_the_gpu():
    """HyperHeun, float64, B = 1, T = 16, the notebook's 7-64-64-64-3 PReLU net: fused against eager gradients on the GPU, and one timing of
    each (printed; the figure in DESIGN.md section 9 is scripts/bench_hyper_train.py's)."""
    import time
    torch.manual_seed(0)
    g = nn.Sequential(nn.Linear(7, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 3)).double().to(DEV)
    t = torch.tensor(GC.GRIDS['uniform16'], dtype=torch.float64, device=DEV)
    y0 = torch.tensor([[1., 1., 1.]], dtype=torch.float64, device=DEV)
    G = torch.randn(16, 1, 3, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    res = {}
    for opt in ('auto', False):
        s = H.HyperHeun(rhs.Lorenz(), g, options={'grad': opt})
        for it in range(3):
            g.zero_grad()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (s.trajectory(t, y0) * G).sum().backward()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        res[opt] = ([p.grad.clone() for p in g.parameters()], dt, s.last_stats['engine'])
    assert res['auto'][2] == 'fused' and res[False][2] == 'eager'
    print('notebook shape, forward + backward: fused %.3f ms, eager %.3f ms' % (1e3 * res['auto'][1], 1e3 * res[False][1]))
    for a, b in zip(res['auto'][0], res[False][0]):
        assert float((a - b).abs().max()) <= GC.F64_BOUND * float(b.abs().max())
