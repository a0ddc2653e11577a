"""Shared inputs of the edge tests of the one-launch hypersolver kernels (csrc/mi_ode_hyper.h: k_hyper_traj, k_hyper_resid, k_hyper_pack): the
cases as data, their systems, nets and time grids, and the restatement runs the GPU tests (tests/test_gpu_hyper_edges.py) compare with.
tests/test_hyper_cases_host.py checks on the CPU that every case can show the defects it is there for, so that a green GPU run means
something and a red one cannot be blamed on the inputs.  Nothing here needs a GPU.

Systems: the four catalogue systems of launch_builtin (Lorenz, Lotka-Volterra, the bias-free 2 x 2 Linear and CubicLinear - autonomous), the
forced oscillator of plugin_examples (time dependent), the same as a plain torch callable that is lowered, and `ring(D)`: a CustomRowLocal
family written as a loop, k[i] = p[0] cos(p[1] t + i) - y[i] + p[2] y[(i + 1) % D] y[(i + D - 1) % D] - time dependent in every component.

Time grids are non-uniform on purpose: the reference steps by dt = t[1] - t[0] everywhere while f sees t[i] of the grid, so neither
t[i + 1] - t[i] nor t0 + i dt reproduces a result.  Horizons are short (8 steps of 0.25; Lorenz,
whose Euler step is unstable at 0.25, 8 steps of 0.05): nothing amplifies rounding differences.

Nets: W = N / sqrt(fan_in), b = 0.3 N, seeded per case (the softplus nets scale their first layer so that pre-activations fall on both sides
of torch's threshold 20 and below -30).  A case's widths are [2 D + 1, hidden .., D]; `acts` has one entry per Linear (the last: an
activation AFTER the last layer), `bias` one flag per Linear.

Bounds (nothing measured on a kernel enters them), on |got - ref| / (1 + |ref|) per element:
  float64   1e-11 against the float64 restatement;
  float32   the reference is the float64 restatement on the float32-rounded inputs, weights and grid; the bound is
            4 x max(E32, bands.case_ceiling(steps, stages = g evaluations per step)), E32 the float32 restatement's own deviation."""
import collections
import functools

import numpy as np
import torch
from torch import nn

from tests import bands
from tests import hyper_restatement as HR

ROWS = 16                       # kHypRows
LD = 129                        # kHypLd
MAX_GRID = 2048                 # kHypMaxGrid
LDS_BUDGET = 160 * 1024         # kHypLdsBudget
WORKSPACE = 1 << 20             # MI_ODE_HYPER_WORKSPACE_BYTES
F64_BOUND = 1e-11

MAIN = (0.3, 0.55, 0.7, 1.3, 1.35, 2.0, 2.25, 2.6, 3.1)          # dt = 0.25 for all eight steps; t[i] far from t0 + i dt
DECREASING = (2.0, 1.75, 1.6, 1.0, 0.95, 0.3, 0.05)              # dt = -0.25
TWO = (0.3, 0.55)
FINE = (0.3, 0.35, 0.37, 0.5, 0.51, 0.6, 0.65, 0.7, 0.8)          # dt = 0.05: Lorenz, whose Euler step is unstable at 0.25
GRIDS = {'main': MAIN, 'fine': FINE, 'decreasing': DECREASING, 'two': TWO, 'four': MAIN[:4], 'three': MAIN[:3]}

TRAJ_OPS = ('euler', 'midpoint', 'heun')
ALL_OPS = TRAJ_OPS + ('resid', 'gresid')
G_EVALS = {'euler': 1, 'midpoint': 2, 'heun': 2, 'resid': 1, 'gresid': 1}

_Case = collections.namedtuple('Case', 'name system D dtype hidden acts bias identity grid B seed first_scale ops')


def Case(name, system, hidden, acts, D=None, dtype='float64', bias=None, identity=False, grid='main', B=37, seed=1, first_scale=1.0, ops=ALL_OPS):
    D = SYSTEMS[system]['D'] if D is None else D
    n = len(hidden) + 1
    acts = tuple(acts) + (None,) * (n - len(acts))
    bias = (True,) * n if bias is None else tuple(bias)
    assert len(acts) == n and len(bias) == n
    return _Case(name, system, D, dtype, tuple(hidden), acts, bias, identity, grid, B, seed, float(first_scale), tuple(ops))


# ---------------------------------------------------------------------------------------------------------------------------------------
# systems
# ---------------------------------------------------------------------------------------------------------------------------------------
W2 = ((-0.1, 2.0), (-2.0, -0.1))
W2C = ((-0.3, 0.8), (-0.8, -0.3))
RING_P = (0.8, 1.7, 0.3)


def ring_body(D):
    return 'for (int i = 0; i < %d; ++i) k[i] = p[0] * cos(p[1] * t + (T)i) - y[i] + p[2] * y[(i + 1) %% %d] * y[(i + %d) %% %d];' % (D, D, D - 1, D)


def ring(D):
    from tfdiffeq_amd import rhs

    def torch_fn(t, y):
        i = torch.arange(D, dtype=y.dtype, device=y.device)
        return RING_P[0] * torch.cos(RING_P[1] * t + i) - y + RING_P[2] * torch.roll(y, -1, -1) * torch.roll(y, 1, -1)
    return rhs.CustomRowLocal(D, ring_body(D), params=list(RING_P), torch_fn=torch_fn)


def _catalogue(name):
    from tfdiffeq_amd import rhs
    if name == 'lorenz':
        return rhs.Lorenz()
    if name == 'lotka':
        return rhs.LotkaVolterra()
    W = torch.tensor(W2, dtype=torch.float64)
    return rhs.Linear(W) if name == 'linear2' else rhs.CubicLinear(torch.tensor(W2C, dtype=torch.float64))


def _forced():
    from tfdiffeq_amd import plugin_examples
    return plugin_examples.forced_oscillator()


# D: the width (None: the case gives it), timed: f uses t, y0: the centre of the initial rows, spread: their standard deviation
SYSTEMS = {
    'lorenz': dict(D=3, timed=False, y0=(1., 1., 1.), spread=0.3, np=lambda D: HR.lorenz, make=lambda D: _catalogue('lorenz'), opts={}),
    'lotka': dict(D=2, timed=False, y0=(1., 1.5), spread=0.2, np=lambda D: HR.lotka_volterra, make=lambda D: _catalogue('lotka'), opts={}),
    'linear2': dict(D=2, timed=False, y0=(1., 0.5), spread=0.3, np=lambda D: HR.linear2(W2), make=lambda D: _catalogue('linear2'), opts={}),
    'cubic2': dict(D=2, timed=False, y0=(1.2, 0.3), spread=0.2, np=lambda D: HR.cubic2(W2C), make=lambda D: _catalogue('cubic2'), opts={}),
    'forced': dict(D=2, timed=True, y0=(1., 0.), spread=0.3, np=lambda D: HR.forced_oscillator, make=lambda D: _forced(), opts={}),
    'forced_lowered': dict(D=2, timed=True, y0=(1., 0.), spread=0.3, np=lambda D: HR.forced_oscillator,
                           make=lambda D: HR.forced_oscillator_torch, opts={'lower': True}),
    'ring': dict(D=None, timed=True, y0=None, spread=0.5, np=lambda D: HR.forced_ring(D, RING_P), make=ring, opts={}),
}


def f_np(case):
    return SYSTEMS[case.system]['np'](case.D)


def make_f(case):
    """(f for the solver's constructor, its options)"""
    s = SYSTEMS[case.system]
    return s['make'](case.D), dict(s['opts'])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
SOFT = 15.0                     # the softplus nets' first layer: pre-activations of standard deviation ~ 10

CASES = [
    # hidden widths 1, 15, 16, 17, 50, 112, 127, 128 with every activation; rows per tile 1, 15, 16, 17, 37
    Case('w1_tanh_b1', 'forced', [1], ['tanh'], B=1),
    Case('w15_relu_b15', 'forced', [15], ['relu'], B=15),
    Case('w16_leaky_b16', 'forced', [16], ['leaky'], B=16),
    Case('w17_prelu_b17', 'forced', [17], ['prelu'], B=17),
    Case('w50_prelu1', 'forced', [50], ['prelu1']),
    Case('w112_tanh', 'forced', [112], ['tanh']),
    Case('w127_softplus', 'forced', [127], ['softplus'], first_scale=SOFT),
    Case('w128_relu', 'forced', [128], ['relu']),
    # layer counts 3 .. 6 (the ping-pong ends in s_b for an odd count), no activation between two Linears, a final Tanh, an Identity,
    # bias-free layers
    Case('l3_none_between', 'forced', [17, 15], ['tanh', None]),
    Case('l4_mixed', 'forced', [16, 17, 15], ['relu', 'leaky', 'prelu']),
    Case('l5_tanh', 'forced', [50, 17, 16, 15], ['tanh', 'prelu1', 'tanh', 'softplus']),
    Case('l6_mixed', 'forced', [17, 16, 15, 17, 16], ['tanh', 'relu', 'leaky', 'prelu', 'tanh']),
    Case('final_tanh', 'forced', [17], ['tanh', 'tanh']),
    Case('identity', 'forced', [16, 17], ['tanh', 'relu'], identity=True),
    Case('nobias_middle', 'forced', [17, 16], ['tanh', 'tanh'], bias=[True, False, True]),
    Case('nobias_last', 'forced', [17], ['leaky'], bias=[True, False]),
    # around the LDS budget
    Case('lds_exact', 'forced', [128, 96], ['tanh', 'tanh']),
    Case('lds_under', 'forced', [112, 96], ['tanh', 'prelu']),
    Case('l2_over', 'forced', [128, 112], ['tanh', 'relu']),
    Case('l2_six', 'forced', [128] * 5, ['tanh', 'prelu', 'tanh', 'leaky', 'tanh']),
    # the other grids
    Case('decreasing', 'forced', [17], ['tanh'], grid='decreasing'),
    Case('two_times', 'forced', [17], ['tanh'], grid='two', B=17),
    # the systems
    Case('lorenz', 'lorenz', [17], ['tanh'], grid='fine'),
    Case('lotka', 'lotka', [16], ['prelu']),
    Case('linear2', 'linear2', [15], ['tanh']),
    Case('cubic2', 'cubic2', [17], ['relu']),
    Case('lowered', 'forced_lowered', [17], ['tanh']),
    Case('ring1', 'ring', [16], ['tanh'], D=1),
    Case('ring7', 'ring', [17], ['tanh'], D=7),                   # 2 D + 1 = 15: one padded input column
    Case('ring8', 'ring', [50], ['prelu'], D=8),                  # 17 of kp0 = 32
    Case('ring16', 'ring', [17], ['tanh'], D=16),                 # the last layer's block full: 16 live columns of 16
    Case('ring17', 'ring', [16], ['relu'], D=17),                 # the last layer over two column blocks, one live column in the second
    Case('ring32', 'ring', [128], ['tanh'], D=32),                # 65 of kp0 = 80, np = 32 all live
    Case('ring32_l2', 'ring', [128, 112], ['tanh', 'tanh'], D=32, B=17),
    # the grid-stride trips
    Case('trip2', 'forced', [16], ['tanh'], grid='four', B=ROWS * MAX_GRID + 1, ops=TRAJ_OPS),
    Case('trip3', 'forced', [16], ['tanh'], grid='four', B=ROWS * 2 * MAX_GRID + 5, ops=('heun',)),
    Case('trip_gresid', 'forced', [16], ['tanh'], grid='three', B=10923, ops=('gresid',)),
    Case('trip_gresid_l2', 'forced', [128, 112], ['tanh', 'tanh'], grid='three', B=10923, ops=('gresid',)),
    Case('trip_resid', 'forced', [16], ['tanh'], grid='three', B=262145, ops=('resid',)),
    # float32
    Case('f32_l4_mixed', 'forced', [16, 17, 15], ['relu', 'leaky', 'prelu'], dtype='float32'),
    Case('f32_w50_prelu1_tanh', 'forced', [50, 17], ['prelu1', 'tanh'], dtype='float32'),
    Case('f32_w127_softplus', 'forced', [127], ['softplus'], dtype='float32', first_scale=SOFT),
    Case('f32_none_final_nobias', 'forced', [16, 15], ['tanh', None, 'tanh'], dtype='float32', bias=[True, False, True]),
    Case('f32_w1', 'forced', [1], ['tanh'], dtype='float32', B=17),
    Case('f32_lds_under', 'forced', [128, 128, 112], ['tanh', 'tanh', 'tanh'], dtype='float32'),
    Case('f32_l2_over', 'forced', [128, 128, 128], ['tanh', 'relu', 'tanh'], dtype='float32'),
    Case('f32_l2_six', 'forced', [128] * 5, ['tanh', 'prelu', 'tanh', 'leaky', 'tanh'], dtype='float32'),
    Case('f32_lotka', 'lotka', [16], ['prelu'], dtype='float32'),
    Case('f32_decreasing', 'forced', [17], ['tanh'], dtype='float32', grid='decreasing'),
    Case('f32_ring8', 'ring', [50], ['prelu'], D=8, dtype='float32'),
    Case('f32_ring32', 'ring', [128], ['tanh'], D=32, dtype='float32'),
    Case('f32_trip_gresid', 'forced', [16], ['tanh'], dtype='float32', grid='three', B=10923, ops=('gresid',)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the budget table of the issue: which side of kHypLdsBudget each net is on
BUDGET = {'lds_exact': 'lds', 'lds_under': 'lds', 'l2_over': 'l2', 'l2_six': 'l2', 'ring32_l2': 'l2', 'trip_gresid_l2': 'l2',
          'f32_lds_under': 'lds', 'f32_l2_over': 'l2', 'f32_l2_six': 'l2'}


def pairs():
    """(case, op) for every parity comparison"""
    return [(c, op) for c in CASES for op in c.ops]


def widths(case):
    return (2 * case.D + 1,) + case.hidden + (case.D,)


def round16(n):
    return (n + 15) // 16 * 16


def pack_elems(case):
    """mi_ode_hyper_run: per layer the [Kp][Np] image of W^T, then b [Np] and a [Np]."""
    w = widths(case)
    return sum(round16(i) * round16(o) + 2 * round16(o) for i, o in zip(w[:-1], w[1:]))


def lds_bytes(case):
    """The dynamic LDS of a network kernel when the weights live there: two activation tiles and the pack."""
    return (2 * ROWS * LD + pack_elems(case)) * np.dtype(case.dtype).itemsize


def path_of(case):
    return 'lds' if lds_bytes(case) <= LDS_BUDGET else 'l2'


def launches_of(case, op):
    """1, or 2 when k_hyper_pack writes the weights to the workspace first (residual_trajectory has no network)."""
    return 2 if op != 'resid' and path_of(case) == 'l2' else 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rounded(case, v):
    v = np.asarray(v, dtype=np.float64)
    return v.astype(np.float32).astype(np.float64) if case.dtype == 'float32' else v


def grid_of(case):
    return _rounded(case, GRIDS[case.grid])


def y0_of(case, B=None):
    """[B, D] in float64 (float32 cases: float32 values).  Row r does not depend on B."""
    s = SYSTEMS[case.system]
    rng = np.random.default_rng(100 + case.seed)
    B = case.B if B is None else B
    centre = np.zeros(case.D) if s['y0'] is None else np.asarray(s['y0'])
    return _rounded(case, centre + s['spread'] * rng.standard_normal((B, case.D)))


def make_g(case, device='cpu'):
    """g as an nn.Sequential in the case's dtype, frozen.  The same parameters on every device: they come from numpy."""
    rng = np.random.default_rng(7000 + 13 * case.seed + sum(widths(case)))
    w = widths(case)
    mods = []
    for l, (i, o) in enumerate(zip(w[:-1], w[1:])):
        lin = nn.Linear(i, o, bias=case.bias[l])
        W = rng.standard_normal((o, i)) / np.sqrt(i) * (case.first_scale if l == 0 else 1.0)
        b = 0.3 * rng.standard_normal(o)
        with torch.no_grad():
            lin.weight.copy_(torch.tensor(W))
            if case.bias[l]:
                lin.bias.copy_(torch.tensor(b))
        mods.append(lin)
        a = case.acts[l]
        if a == 'relu':
            mods.append(nn.ReLU())
        elif a == 'leaky':
            mods.append(nn.LeakyReLU(0.2))
        elif a in ('prelu', 'prelu1'):
            m = nn.PReLU(o if a == 'prelu' else 1)
            with torch.no_grad():
                m.weight.copy_(torch.tensor(rng.uniform(0.05, 0.5, o if a == 'prelu' else 1)))      # per channel: distinct
            mods.append(m)
        elif a == 'tanh':
            mods.append(nn.Tanh())
        elif a == 'softplus':
            mods.append(nn.Softplus())
        else:
            assert a is None
        if case.identity and l == 0:
            mods.append(nn.Identity())
    return nn.Sequential(*mods).to(device=device, dtype=getattr(torch, case.dtype)).requires_grad_(False)


@functools.lru_cache(maxsize=None)
def layers_of(case):
    """g's layers as float64 arrays: the float64 net's own, or the float32 net's values widened (the LeakyReLU slope rounded as well)."""
    g = make_g(case)
    return HR.g_layers_f32(g) if case.dtype == 'float32' else HR.g_layers(g)


@functools.lru_cache(maxsize=None)
def base_of(case):
    """The given trajectory of the residual modes: the float64 restatement's HyperEuler trajectory, each row moved by 0.05 N so that the
    recovered residual is not g itself."""
    traj = HR.trajectory('euler', f_np(case), layers_of(case), grid_of(case), y0_of(case))
    return _rounded(case, traj + 0.05 * np.random.default_rng(300 + case.seed).standard_normal(traj.shape))


# ---------------------------------------------------------------------------------------------------------------------------------------
# restatement runs
# ---------------------------------------------------------------------------------------------------------------------------------------
def restate(case, op, dtype='float64', f=None, layers=None, pre=None):
    f = f_np(case) if f is None else f
    layers = layers_of(case) if layers is None else layers
    t = grid_of(case)
    if op in TRAJ_OPS:
        return HR.trajectory(op, f, layers, t, y0_of(case), dtype=dtype, pre=pre)
    if op == 'resid':
        return HR.residual_trajectory(f, t, base_of(case), dtype=dtype)
    return HR.hypersolver_residuals(f, layers, t, base_of(case), dtype=dtype, pre=pre)


@functools.lru_cache(maxsize=None)
def reference(case, op):
    """The comparison target, float64.  Shared by the tests: do not write to it."""
    out = restate(case, op)
    out.setflags(write=False)
    return out


def steps_of(case, op):
    return 1 if op == 'gresid' else len(GRIDS[case.grid]) - 1      # (a row of _hypersolver_residuals is one evaluation: nothing accumulates)


@functools.lru_cache(maxsize=None)
def e32(case, op):
    """The float32 restatement's own deviation from the reference."""
    return bands.observed(restate(case, op, dtype='float32'), reference(case, op))


def bound_of(case, op):
    if case.dtype == 'float64':
        return F64_BOUND
    return 4.0 * max(e32(case, op), bands.case_ceiling(steps_of(case, op), stages=G_EVALS[op]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# wrong on purpose: what the inputs must be able to tell from the right result (tests/test_hyper_cases_host.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
def frozen_t(f, t0):
    return lambda t, y: f(t0, y)


def zeroed_last(layers):
    out = [list(l) for l in layers]
    out[-1][0] = np.zeros_like(out[-1][0])
    out[-1][1] = None
    return out


def wrong_trajectory(variant, method, f, layers, t, y0):
    """HR.trajectory in float64 with one defect: 'stage_time' (midpoint's second evaluation at t + dt, Heun's at t + dt / 2), 'local_dt'
    (the step t[i + 1] - t[i]), 'dt2' (the second correction scaled by dt^2)."""
    assert variant in ('stage_time', 'local_dt', 'dt2') and (method != 'euler' or variant == 'local_dt')
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y0, dtype=np.float64)
    traj = []
    for i in range(len(t)):
        traj.append(y)
        if i == len(t) - 1:
            break
        dt = t[i + 1] - t[i] if variant == 'local_dt' else t[1] - t[0]
        p2 = dt * dt if variant == 'dt2' else dt * dt * dt
        dy = f(t[i], y)
        if method == 'euler':
            y = y + dy * dt + dt * dt * HR.hyper_g(layers, dt, y, dy)
        elif method == 'midpoint':
            y_mid = y + dy * dt / 2. + dt * dt * HR.hyper_g(layers, dt, y, dy)
            dy2 = f(t[i] + (dt if variant == 'stage_time' else dt / 2.), y_mid)
            y = y + dt * dy2 + p2 * HR.hyper_g(layers, dt, y_mid, dy2)
        else:
            y2 = y + dy * dt + dt * dt * HR.hyper_g(layers, dt, y, dy)
            dy2 = f(t[i] + (dt / 2. if variant == 'stage_time' else dt), y2)
            y = y + dt / 2. * (dy + dy2) + p2 * HR.hyper_g(layers, dt, y2, dy2)
    return np.stack(traj)


def uniform(case):
    g = np.asarray(GRIDS[case.grid])
    return len(g) == 2 or bool(np.allclose(np.diff(g), g[1] - g[0]))


def variants_of(case, op):
    """The defects (case, op) must be able to show."""
    timed = SYSTEMS[case.system]['timed']
    out = []
    if timed and (len(GRIDS[case.grid]) > 2 or op not in ('euler', 'resid')):       # (one Euler step sees t[0] only)
        out.append('t0')
    if op in ('midpoint', 'heun'):
        out.append('dt2')
        if timed:
            out.append('stage_time')
    if op in TRAJ_OPS and not uniform(case):
        out.append('local_dt')
    if op != 'resid':
        out.append('g0')
    return out


def wrong(case, op, variant):
    f, layers, t = f_np(case), layers_of(case), grid_of(case)
    if variant == 't0':
        return restate(case, op, f=frozen_t(f, t[0]))
    if variant == 'g0':
        return restate(case, op, layers=zeroed_last(layers))
    return wrong_trajectory(variant, op, f, layers, t, y0_of(case))


# ---------------------------------------------------------------------------------------------------------------------------------------
# prebuilding
# ---------------------------------------------------------------------------------------------------------------------------------------
def hyper_sources():
    """Every hyper plugin source (csrc/mi_ode_hyper_plugin.h) the cases compile: what __graft_entry__.build() puts in the in-tree cache."""
    from tfdiffeq_amd import hyper_solvers
    out = []
    for system, D, dtype in sorted(set((c.system, c.D, c.dtype) for c in CASES)):
        td = getattr(torch, dtype)
        f = SYSTEMS[system]['make'](D)
        for s in hyper_solvers.hyper_sources(f, torch.zeros(2, D, dtype=td), dtype=td):
            if s not in out:
                out.append(s)
    return out
