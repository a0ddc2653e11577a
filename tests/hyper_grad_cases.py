"""Shared inputs of the tests of the fused hypersolver gradient (csrc/mi_ode_hyper_grad.h; tests/test_hyper_grad_host.py on the CPU,
tests/test_gpu_hyper_grad.py on the GPU): the cases as data, their systems, nets, grids and cotangents, and the yardstick - the package's
own eager loop on the CPU in float64 under torch autograd, on the float32-rounded inputs for a float32 case.  Nothing here needs a GPU.

loss = (out * G).sum(), G seeded.  Metric per gradient tensor: max|got - ref| / max|ref|; where ref is exactly zero, got must be too.
Bounds (nothing measured on the kernel enters them):
  float64   1e-11 (the hypersolver suite's F64_BOUND; reordering rows and hidden units moves the oracle's own gradients by <= 6e-16);
  float32   4 x max(E32, bands.case_ceiling(steps, stages = 2 x g evaluations per step)), E32 the deviation of the float32 CPU eager
            gradients from their float64 twin.
Kinked activations (ReLU / LeakyReLU / PReLU): a float32 case is admitted only if no pre-activation of the float64 oracle run lies
within 1e-4 of 0 (such cases are tiny, their seed is fixed here); a float64 case asserts a margin of 1e-9.

Nets: W = N / sqrt(fan_in), b = 0.3 N, PReLU weights 0.25 + 0.1 N, seeded per case; `first_scale` multiplies the first layer (Softplus:
pre-activations on both sides of torch's threshold 20 and below -30)."""
import collections
import functools

import numpy as np
import torch
from torch import nn

from tests import bands
from tests import hyper_restatement as HR

F64_BOUND = 1e-11
KINK_F32, KINK_F64 = 1e-4, 1e-9
DEFAULT_GRID = 128              # hyper_solvers.GRAD_DEFAULT_GRID

MAIN = (0.3, 0.55, 0.7, 1.3, 1.35, 2.0, 2.25, 2.6, 3.1)          # dt = 0.25 for every step; t[i] far from t0 + i dt
FINE = (0.3, 0.35, 0.37, 0.5, 0.51, 0.6, 0.65, 0.7, 0.8)          # dt = 0.05: Lorenz
GRIDS = {'main9': MAIN, 'main3': MAIN[:3], 'main2': MAIN[:2], 'fine9': FINE, 'fine3': FINE[:3], 'fine2': FINE[:2],
         'dec9': tuple(2.3 - v for v in MAIN), 'decfine3': tuple(1.1 - v for v in FINE[:3]), 'decfine9': tuple(1.1 - v for v in FINE),
         'uniform16': tuple(0.01 * i for i in range(16))}

METHODS = ('euler', 'midpoint', 'heun')
G_EVALS = {'euler': 1, 'midpoint': 2, 'heun': 2, 'gresid': 1}

_Case = collections.namedtuple('Case', 'name system op dtype hidden acts bias identity grid B seed first_scale grad_grid cot leaves')


def Case(name, system, op, hidden, acts, dtype='float64', bias=None, identity=False, grid=None, B=17, seed=1, first_scale=1.0, grad_grid=0,
         cot='all', leaves='all'):
    n = len(hidden) + 1
    acts = tuple(acts) + (None,) * (n - len(acts))
    bias = (True,) * n if bias is None else tuple(bias)
    assert len(acts) == n and len(bias) == n
    if grid is None:
        grid = 'fine3' if SYSTEMS[system]['fine'] else 'main3'
    return _Case(name, system, op, dtype, tuple(hidden), acts, bias, identity, grid, B, seed, float(first_scale), grad_grid, cot, leaves)


def time_dependent_torch(t, y):
    """A plain Python callable that uses t, of width 3 (lowered onto a generated row-local kernel with a generated vjp)."""
    return torch.stack([y[..., 1] * torch.cos(1.3 * t), 0.7 * torch.sin(2.0 * t) - y[..., 0] * y[..., 2], t * y[..., 0] - 0.5 * y[..., 2]], dim=-1)


def _rhs(name):
    from tfdiffeq_amd import rhs
    return rhs.Lorenz() if name == 'lorenz' else rhs.LotkaVolterra()


SYSTEMS = {
    'lorenz': dict(D=3, fine=True, y0=(1., 1., 1.), spread=0.3, make=lambda: _rhs('lorenz')),
    'lotka': dict(D=2, fine=False, y0=(1., 1.5), spread=0.2, make=lambda: _rhs('lotka')),
    'lorenz_lowered': dict(D=3, fine=True, y0=(1., 1., 1.), spread=0.3, make=lambda: HR.lorenz_torch),
    'forced': dict(D=2, fine=False, y0=(1., 0.), spread=0.3, make=lambda: HR.forced_oscillator_torch),
    'timed3': dict(D=3, fine=False, y0=(0.5, -0.3, 0.8), spread=0.3, make=lambda: time_dependent_torch),
}

SOFT = 15.0
NOTEBOOK = [64, 64, 64]

CASES = [
    # rows per tile and tiles per workgroup
    Case('b1', 'lorenz', 'heun', [17], ['tanh'], B=1),
    Case('b15', 'lotka', 'euler', [17], ['tanh'], B=15),
    Case('b16', 'lorenz', 'midpoint', [17], ['tanh'], B=16),
    Case('b17', 'lotka', 'heun', [17], ['tanh'], B=17),
    Case('b37', 'lorenz', 'heun', [17], ['tanh'], B=37, grid='fine9'),
    Case('b37_grid2', 'lorenz', 'heun', [17], ['tanh'], B=37, grid='fine9', grad_grid=2),
    Case('b37_grid1', 'lotka', 'midpoint', [17], ['prelu'], B=37, grid='main9', grad_grid=1),
    Case('default_grid', 'lotka', 'heun', [16], ['tanh'], B=16 * DEFAULT_GRID + 5),
    # hidden widths; first layer 2 D + 1 = 5 and 7; last layer D < 16
    Case('w1', 'lorenz', 'heun', [1], ['tanh']),
    Case('w15', 'lotka', 'euler', [15], ['relu']),
    Case('w16', 'lorenz', 'midpoint', [16], ['leaky']),
    Case('w17', 'lotka', 'heun', [17], ['prelu']),
    Case('w50', 'lorenz', 'euler', [50], ['prelu1']),
    Case('w64', 'lotka', 'midpoint', [64], ['tanh']),
    Case('w127', 'lorenz', 'heun', [127], ['softplus'], first_scale=SOFT),
    Case('w128', 'lotka', 'heun', [128], ['relu']),
    # layers and activations
    Case('l3_none_between', 'lorenz', 'heun', [17, 15], ['tanh', None]),
    Case('l4_mixed', 'lotka', 'heun', [16, 17, 15], ['relu', 'leaky', 'prelu']),
    Case('final_tanh', 'lorenz', 'midpoint', [17], ['tanh', 'tanh']),
    Case('identity', 'lotka', 'euler', [16, 17], ['tanh', 'softplus'], identity=True),
    Case('nobias_middle', 'lorenz', 'heun', [17, 16], ['tanh', 'tanh'], bias=[True, False, True]),
    Case('nobias_last', 'lotka', 'midpoint', [17], ['leaky'], bias=[True, False]),
    Case('prelu1_l3', 'lorenz', 'heun', [17, 33], ['prelu1', 'prelu']),
    # weight paths: images in LDS (everything above), the packed global image (two launches)
    Case('packed_128', 'lorenz', 'heun', [128, 128], ['softplus', 'tanh']),
    Case('packed_notebook', 'lorenz', 'heun', NOTEBOOK, ['prelu1', 'prelu1', 'prelu1'], B=3),
    Case('l4_64', 'lotka', 'midpoint', [64, 64, 64], ['tanh', 'tanh', 'tanh'], dtype='float32'),
    # operations: the three methods and _hypersolver_residuals in both dtypes, the grids, the systems
    Case('euler9', 'lorenz', 'euler', [17], ['tanh'], B=37, grid='fine9'),
    Case('midpoint9', 'lotka', 'midpoint', [17], ['tanh'], B=37, grid='main9'),
    Case('gresid', 'lorenz', 'gresid', [17], ['tanh'], B=37, grid='fine9'),
    Case('gresid_grid2', 'lotka', 'gresid', [17], ['prelu1'], B=7, grid='main9', grad_grid=2),
    Case('decreasing', 'lorenz', 'heun', [17], ['tanh'], grid='decfine9'),
    Case('decreasing_timed', 'forced', 'midpoint', [17], ['tanh'], grid='dec9'),
    Case('timed_euler', 'forced', 'euler', [16], ['tanh'], grid='main9'),
    Case('timed_heun', 'timed3', 'heun', [17], ['tanh'], grid='main9'),
    Case('timed_gresid', 'timed3', 'gresid', [17], ['tanh'], grid='main9'),
    Case('two_times', 'forced', 'heun', [17], ['tanh'], grid='main2'),
    Case('lowered_lorenz', 'lorenz_lowered', 'heun', [17], ['tanh'], B=37, grid='fine9'),
    # float32: smooth nets carry the shapes, kinked ones are tiny
    Case('f32_euler', 'lorenz', 'euler', [17], ['tanh'], dtype='float32', B=37, grid='fine9'),
    Case('f32_midpoint', 'lotka', 'midpoint', [50], ['tanh'], dtype='float32', B=37, grid='main9'),
    Case('f32_heun', 'lorenz', 'heun', [127], ['softplus'], dtype='float32', B=37, grid='fine9', first_scale=SOFT),
    Case('f32_gresid', 'forced', 'gresid', [17, 16], ['tanh', 'softplus'], dtype='float32', B=37, grid='main9'),
    Case('f32_timed', 'timed3', 'heun', [16], ['tanh'], dtype='float32', grid='main9'),
    Case('f32_decreasing', 'lorenz', 'midpoint', [17], ['tanh'], dtype='float32', grid='decfine3'),
    Case('f32_packed_128', 'lotka', 'heun', [128, 128, 128], ['tanh', 'softplus', 'tanh'], dtype='float32'),
    Case('f32_grid2', 'lorenz', 'heun', [17], ['tanh'], dtype='float32', B=37, grid='fine9', grad_grid=2),
    Case('f32_kink_relu', 'lotka', 'heun', [15], ['relu'], dtype='float32', B=4, seed=3),
    Case('f32_kink_prelu', 'lorenz', 'midpoint', [17], ['prelu'], dtype='float32', B=3, seed=3),
    Case('f32_kink_leaky_prelu1', 'lotka', 'euler', [16, 17], ['leaky', 'prelu1'], dtype='float32', B=4, seed=3),
    # cotangents
    Case('cot_last', 'lorenz', 'heun', [17], ['tanh'], cot='last'),
    Case('cot_row0', 'lotka', 'heun', [17], ['prelu'], cot='row0'),
    Case('cot_noncontig', 'lorenz', 'midpoint', [17], ['tanh'], cot='noncontig'),
    # which leaves
    Case('leaves_last', 'lorenz', 'heun', [17, 16], ['tanh', 'prelu'], leaves='last'),
    Case('leaves_bias', 'lotka', 'midpoint', [17, 16], ['tanh', 'prelu'], leaves='bias'),
    Case('leaves_y0', 'lorenz', 'heun', [17], ['tanh'], leaves='y0'),
    Case('leaves_g', 'lotka', 'euler', [17], ['tanh'], leaves='g'),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
KINKED = ('relu', 'leaky', 'prelu', 'prelu1')


def torch_dtype(case):
    return getattr(torch, case.dtype)


def dim_of(case):
    return SYSTEMS[case.system]['D']


def make_f(case):
    return SYSTEMS[case.system]['make']()


def grid_of(case):
    g = np.asarray(GRIDS[case.grid], dtype=np.float64)
    return g.astype(np.float32).astype(np.float64) if case.dtype == 'float32' else g


def steps_of(case):
    return len(GRIDS[case.grid]) - 1 if case.op != 'gresid' else 1


def _round(case, x):
    return x.astype(np.float32).astype(np.float64) if case.dtype == 'float32' else x


def y0_of(case):
    s = SYSTEMS[case.system]
    rng = np.random.default_rng(1000 + case.seed)
    return _round(case, np.asarray(s['y0'])[None, :] + s['spread'] * rng.standard_normal((case.B, len(s['y0']))))


def base_of(case):
    """The base trajectory of a gresid case: rows around the system's centre, one block per time."""
    s = SYSTEMS[case.system]
    rng = np.random.default_rng(2000 + case.seed)
    T = len(GRIDS[case.grid])
    return _round(case, np.asarray(s['y0'])[None, None, :] + s['spread'] * rng.standard_normal((T, case.B, len(s['y0']))))


def cotangent_of(case):
    rng = np.random.default_rng(3000 + case.seed)
    T = len(GRIDS[case.grid])
    return _round(case, rng.standard_normal((T, case.B, dim_of(case))))


_ACT = {'relu': lambda w: nn.ReLU(), 'leaky': lambda w: nn.LeakyReLU(0.2), 'prelu': lambda w: nn.PReLU(w), 'prelu1': lambda w: nn.PReLU(1),
        'tanh': lambda w: nn.Tanh(), 'softplus': lambda w: nn.Softplus()}


def make_g(case, dtype=None, device='cpu'):
    """g with the case's seeded weights (rounded to float32 for a float32 case) in `dtype` (default: the case's), every parameter trainable."""
    D = dim_of(case)
    widths = [2 * D + 1] + list(case.hidden) + [D]
    rng = np.random.default_rng(4000 + case.seed)
    mods = []
    for j in range(len(widths) - 1):
        lin = nn.Linear(widths[j], widths[j + 1], bias=case.bias[j])
        W = rng.standard_normal((widths[j + 1], widths[j])) / np.sqrt(widths[j]) * (case.first_scale if j == 0 else 1.0)
        b = 0.3 * rng.standard_normal(widths[j + 1])
        with torch.no_grad():
            lin.weight.copy_(torch.tensor(_round(case, W)))
            if case.bias[j]:
                lin.bias.copy_(torch.tensor(_round(case, b)))
        mods.append(lin)
        if case.identity and j == 0:
            mods.append(nn.Identity())
        if case.acts[j] is not None:
            act = _ACT[case.acts[j]](widths[j + 1])
            if isinstance(act, nn.PReLU):
                with torch.no_grad():
                    act.weight.copy_(torch.tensor(_round(case, 0.25 + 0.1 * rng.standard_normal(act.num_parameters))))
            mods.append(act)
    g = nn.Sequential(*mods).to(dtype=dtype or torch_dtype(case), device=device)
    return g


def set_leaves(case, g):
    """requires_grad of g's parameters as the case says; True when y0 is a leaf."""
    linears = [m for m in g if isinstance(m, nn.Linear)]
    for name, p in g.named_parameters():
        if case.leaves in ('all', 'g'):
            p.requires_grad_(True)
        elif case.leaves == 'y0':
            p.requires_grad_(False)
        elif case.leaves == 'bias':
            p.requires_grad_(name.endswith('bias'))
        elif case.leaves == 'last':
            p.requires_grad_(any(p is q for q in linears[-1].parameters()))
    return case.leaves in ('all', 'y0') and case.op != 'gresid'


def solver_of(case, f, g, options=None):
    from tfdiffeq_amd import hyper_solvers as H
    cls = {'euler': H.HyperEuler, 'midpoint': H.HyperMidpoint, 'heun': H.HyperHeun, 'gresid': H.HyperEuler}[case.op]
    return cls(f, g, options=options)


def call(case, solver, t, y):
    return solver._hypersolver_residuals(t, y) if case.op == 'gresid' else solver.trajectory(t, y)


def loss_of(case, out, G):
    """(out * G).sum() with the case's cotangent: everywhere, on the last row, on row 0, or through a non-contiguous G."""
    if case.cot == 'last':
        return (out[-1] * G[-1]).sum()
    if case.cot == 'row0':
        return (out[0] * G[0]).sum()
    if case.cot == 'noncontig':
        return (out * G.permute(2, 1, 0).contiguous().permute(2, 1, 0)).sum()
    return (out * G).sum()


def run(case, dtype, device='cpu', options=None, eager=False, pre=None):
    """One forward and backward of the case in `dtype` on `device`: (out, {'y0': grad | None, 'params': [grad | None per parameter of g]},
    solver).  eager: the package's eager loop directly (the yardstick; works on CPU tensors).  pre: a list that receives the
    pre-activation of every Linear that a kinked activation follows."""
    from tfdiffeq_amd import _native as N
    f = make_f(case)
    g = make_g(case, dtype=dtype, device=device)
    y_leaf = set_leaves(case, g)
    if pre is not None:
        mods = list(g)
        for a, b in zip(mods, mods[1:] + [None]):
            if isinstance(a, nn.Linear) and isinstance(b, (nn.ReLU, nn.LeakyReLU, nn.PReLU)):
                a.register_forward_hook(lambda m, i, o: pre.append(o.detach().clone()))
    solver = solver_of(case, f, g, options)
    t = torch.tensor(grid_of(case), dtype=dtype, device=device)
    y = torch.tensor(base_of(case) if case.op == 'gresid' else y0_of(case), dtype=dtype, device=device).requires_grad_(y_leaf)
    G = torch.tensor(cotangent_of(case), dtype=dtype, device=device)
    if eager:
        out = solver._eager(N.HYPER_G_RESIDUALS if case.op == 'gresid' else N.HYPER_TRAJECTORY, t, y)
    else:
        out = call(case, solver, t, y)
    loss_of(case, out, G).backward()
    leaf = dict([('y0', y_leaf)] + [('p%d' % i, p.requires_grad) for i, p in enumerate(g.parameters())])
    return out.detach(), {'y0': y.grad, 'params': [p.grad for p in g.parameters()], 'leaf': leaf}, solver


@functools.lru_cache(maxsize=None)
def _oracle(name):
    case = BY_NAME[name]
    pre = []
    out, grads, _ = run(case, torch.float64, eager=True, pre=pre)
    margin = min([float(z.abs().min()) for z in pre]) if pre else float('inf')
    return out, grads, margin


def oracle(case):
    """(out, grads, the smallest |pre-activation| in front of a kinked activation) of the float64 CPU eager run; computed once, shared, never
    changed by a test."""
    return _oracle(case.name)


@functools.lru_cache(maxsize=None)
def _e32(name):
    case = BY_NAME[name]
    _, ref, _ = oracle(case)
    _, got, _ = run(case, torch.float32, eager=True)
    return max(deviations(got, ref).values())


def deviations(got, ref):
    """{tensor name: max|got - ref| / max|ref|}; a tensor whose reference is exactly zero must be exactly zero (deviation 0 or inf); a
    tensor the reference has no gradient for must have none."""
    out = {}
    pairs = [('y0', got['y0'], ref['y0'])] + [('p%d' % i, a, b) for i, (a, b) in enumerate(zip(got['params'], ref['params']))]
    assert len(got['params']) == len(ref['params'])
    leaf = got.get('leaf', {})
    for name, a, b in pairs:
        if b is None:                                    # no path from the tensor to the loss, or not a leaf: nothing, or exact zeros
            assert a is None or (leaf.get(name, False) and float(a.abs().max()) == 0.0), '%s: a gradient where the yardstick has none' % name
            continue
        assert a is not None, '%s: no gradient' % name
        a, b = a.detach().cpu().double(), b.detach().cpu().double()
        assert a.shape == b.shape, (name, a.shape, b.shape)
        scale = float(b.abs().max())
        if scale == 0.0:
            out[name] = 0.0 if float(a.abs().max()) == 0.0 else float('inf')
        else:
            out[name] = float((a - b).abs().max()) / scale
    return out


def e32(case):
    return _e32(case.name)


def bound_of(case):
    if case.dtype == 'float64':
        return F64_BOUND
    return 4 * max(e32(case), bands.case_ceiling(steps_of(case), stages=2 * G_EVALS[case.op]))


def is_kinked(case):
    return any(a in KINKED for a in case.acts)


def sources():
    """The hyper-grad plugin translation units of every case and the hyper plugins of the lowered callables' forward calls (build-time
    prebuilding: the GPU machine compiles nothing), deduplicated."""
    from tfdiffeq_amd import hyper_solvers as H
    out = []
    for c in CASES:
        y = torch.tensor(y0_of(c)[:2], dtype=torch_dtype(c))
        for s in H.hyper_grad_sources(make_f(c), y) + H.hyper_sources(make_f(c), y):
            if s not in out:
                out.append(s)
    return out
