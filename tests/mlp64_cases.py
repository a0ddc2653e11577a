"""Shared inputs of the float64 MLP tile-kernel tests (csrc/mi_ode_mlp64.h): the network builder, its numpy restatement, the case tables and
the oracle runs the GPU tests compare with.  tests/test_mlp64_cases_host.py checks on the CPU that the cases have the properties the GPU
tests (tests/test_gpu_mlp64_edges.py) rely on - rejected attempts, error ratios away from 1, several output times inside one step - so that
a GPU failure cannot be blamed on the inputs.  Nothing here needs a GPU; torch is imported only where a device object is built.

Batches that depend on the device are functions of its compute-unit count (the grid of the tile kernels is min(CUs, ceil(batch / 32))
workgroups): B2 = 32 * cus + 33 - two workgroups make a second trip and the last tile has ONE row; B3 = 64 * cus + 1 - every workgroup makes
a second trip and one a third, of one row."""
import collections
import contextlib
import functools

import numpy as np

DEFAULT_CUS = 256
TILE = 32


def B2(cus=DEFAULT_CUS):
    return TILE * cus + 33


def B3(cus=DEFAULT_CUS):
    return 2 * TILE * cus + 1


def n_tiles(batch):
    return -(-batch // TILE)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the network and its numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def make_net(d, h, seed, td=False, bias=True, gain=1.0):
    """[W1, b1, W2, b2, W3, b3] in float64 numpy, [in, out] layout: W / sqrt(fan_in) (the middle layer times `gain`), biases 0.1 * randn or
    None, with td a time row in front of W1 (dense_odenet.py:79-84)."""
    rng = np.random.default_rng(seed)
    W1 = rng.standard_normal((d + (1 if td else 0), h)) / np.sqrt(d)
    W2 = gain * rng.standard_normal((h, h)) / np.sqrt(h)
    W3 = rng.standard_normal((h, d)) / np.sqrt(h)
    b1, b2, b3 = (0.1 * rng.standard_normal(n) for n in (h, h, d))
    return [W1, b1, W2, b2, W3, b3] if bias else [W1, None, W2, None, W3, None]


ACTS = {'tanh': np.tanh, 'relu': lambda x: np.maximum(x, 0.0), 'softplus': lambda x: np.logaddexp(x, 0.0)}


def np_f(ws, act, td):
    """f(t, y) of the network in numpy float64."""
    W1, b1, W2, b2, W3, b3 = ws
    a = ACTS[act]

    def lin(x, W, b):
        return x @ W if b is None else x @ W + b

    def f(t, y):
        x = np.concatenate([np.full(y.shape[:-1] + (1,), t, dtype=y.dtype), y], -1) if td else y
        with np.errstate(over='ignore'):
            return lin(a(lin(a(lin(x, W1, b1)), W2, b2)), W3, b3)
    return f


def to_mlp(ws, act, td, device):
    """The same network as a device descriptor (tfdiffeq_amd.rhs.MLP)."""
    import torch
    from tfdiffeq_amd import rhs
    dev = [None if w is None else torch.tensor(w, dtype=torch.float64, device=device) for w in ws]
    return rhs.MLP(*dev, activation=act, time_dependent=td)


def make_y0(batch, d, seed, spread=1.0):
    """spread 1: independent standard normal rows.  spread < 1: one standard normal row plus spread * randn per row - a batch that moves
    together, so that the batch-wide error ratio (a MEAN over all rows, misc.py:262) follows one trajectory's error instead of averaging the
    rows' fluctuations away: what makes the controller reject (with independent rows the oracle accepted every attempt at any stiffness)."""
    rng = np.random.default_rng(seed + 1000)
    if spread == 1.0:
        return rng.standard_normal((batch, d))
    return rng.standard_normal((1, d)) + spread * rng.standard_normal((batch, d))


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
_Case = collections.namedtuple('Case', 'name d h act td bias seed gain spread method t rtol atol batch first_step rejecting options')


def Case(name, d, h, act, method, t, batch, td=False, bias=True, seed=1, gain=1.0, spread=1.0, rtol=1e-6, atol=1e-8, first_step=None,
         rejecting=False, options=None):
    return _Case(name, d, h, act, td, bias, seed, gain, spread, method, tuple(float(x) for x in t), rtol, atol, batch, first_step, rejecting, options)


def batch_of(case, cus=DEFAULT_CUS):
    return {'B2': B2, 'B3': B3}[case.batch](cus) if isinstance(case.batch, str) else case.batch


def tol_of(case):
    """The project's float64 bars for these kernels: 1e-9 absolute against the oracle, 1e-7 for dopri8, 1e-11 on a fixed grid."""
    if case.method in ('euler', 'rk4'):
        return 1e-11
    return 1e-7 if case.method == 'dopri8' else 1e-9


G64, G16 = (64, 128), (6, 16)
T_FWD, T_REV = (0., 0.12, 0.3), (0.3, 0.12, 0.)
# a stiff middle layer and a batch that moves together: the oracle rejects (REJ for tanh; the unbounded activations grow, so less gain)
REJ = dict(gain=40.0, spread=0.01, rejecting=True)
REJ_U = dict(gain=8.0, spread=0.01, rejecting=True)


def _multi(geom, tag):
    d, h = geom
    # (bosh3's tolerances are the existing file's)
    return [
        Case(tag + '-dopri5-B2', d, h, 'tanh', 'dopri5', T_FWD, 'B2', seed=11, **REJ),
        Case(tag + '-dopri5-B3-td', d, h, 'relu', 'dopri5', T_FWD, 'B3', td=True, seed=12, **REJ_U),
        Case(tag + '-tsit5-B2-td', d, h, 'softplus', 'tsit5', T_FWD, 'B2', td=True, seed=13, **REJ_U),
        Case(tag + '-bosh3-B2-rev', d, h, 'tanh', 'bosh3', T_REV, 'B2', seed=14, rtol=1e-4, atol=1e-6, **REJ),
        Case(tag + '-dopri8-B2', d, h, 'tanh', 'dopri8', T_FWD, 'B2', seed=15, **REJ),
    ]


MULTI_ADAPTIVE = _multi(G64, 'g64') + _multi(G16, 'g16')

GRID_UP = (0., 0.25, 0.5, 0.75)
GRID_DOWN = (1.0, 0.8, 0.3, 0.25)                 # decreasing, non-uniform
MULTI_FIXED = [Case('%s-%s-%s' % (tag, method, gname), d, h, act, method, grid, 'B2', td=td, seed=21 + i)
               for i, ((d, h), tag) in enumerate(((G64, 'g64'), (G16, 'g16')))
               for method, act, td in (('euler', 'tanh', True), ('rk4', 'softplus', False))
               for gname, grid in (('up', GRID_UP), ('down', GRID_DOWN))]

# (dim, hidden): the geometry choice's edges.  16 x 16 serves dim <= 16 and hidden <= 16 TOGETHER; (16, 17) and (17, 16) must fall to 64 x 128.
WIDTHS = [(1, 1), (1, 128), (64, 1), (15, 15), (16, 17), (17, 16), (17, 17), (63, 127), (5, 101), (64, 128)]
_ROT = ['tanh', 'relu', 'softplus']
WIDTH_EDGES = [Case('w%dx%d' % (d, h), d, h, _ROT[i % 3], 'dopri5', T_FWD, 65, td=(i % 2 == 1), bias=(d, h) not in ((15, 15), (63, 127)),
                    seed=31 + i, gain=2.0)
               for i, (d, h) in enumerate(WIDTHS)]

# fusion='step' against the whole-call kernel (bit identical), and both against the oracle
SCHEDULES = [
    Case('s-bosh3', 64, 128, 'tanh', 'bosh3', T_FWD, 300, seed=41, rtol=1e-4, atol=1e-6, **REJ),
    Case('s-tsit5', 64, 128, 'softplus', 'tsit5', T_FWD, 300, seed=42, **REJ_U),
    Case('s-dopri8', 64, 128, 'tanh', 'dopri8', T_FWD, 300, seed=43, **REJ),
    Case('s-g16-dopri5', 6, 16, 'tanh', 'dopri5', T_FWD, 300, seed=44, **REJ),
    Case('s-g16-tsit5', 6, 16, 'relu', 'tsit5', T_FWD, 300, seed=45, gain=3.0),
    Case('s-td', 64, 128, 'tanh', 'dopri5', T_FWD, 300, td=True, seed=46, **REJ),
    Case('s-rev', 64, 128, 'relu', 'dopri5', T_REV, 300, seed=47, gain=3.0),
    MULTI_ADAPTIVE[0],                                     # g64-dopri5-B2: more than one tile per workgroup under fusion='step'
    Case('s-first-step', 64, 128, 'tanh', 'dopri5', T_FWD, 300, seed=48, gain=3.0, first_step=0.01),
    Case('s-g16-first-step', 6, 16, 'softplus', 'tsit5', T_FWD, 300, td=True, seed=49, gain=3.0, first_step=0.01),
]

# 40 output times: 36 of them inside [0.2, 0.26] (several per accepted step), two 1e-12 apart
T_DENSE = (0.,) + tuple(np.linspace(0.2, 0.26, 36)) + (0.4, 0.4 + 1e-12, 1.0)
DENSE = [Case('dense-%s-%s' % (tag, method), d, h, act, method, T_DENSE, 33, td=td, seed=51 + i, gain=2.0)
         for i, ((d, h), tag, act, td) in enumerate(((G64, 'g64', 'tanh', False), (G16, 'g16', 'softplus', True)))
         for method in ('dopri5', 'tsit5')]

# fixed-grid options: outputs strictly between the points of a step_size grid, and eps (the oracle takes both)
FIXED_OPTIONS = [Case('fo-%s-%s-%s' % (tag, act, oname), d, h, act, method, (0., 0.33, 0.7), 77, td=(act == 'relu'), seed=61 + i, options=opt)
                 for i, ((d, h), tag) in enumerate(((G16, 'g16'), (G64, 'g64')))
                 for act, method in (('relu', 'rk4'), ('softplus', 'euler'))
                 for oname, opt in (('step', (('step_size', 0.1),)), ('eps', (('eps', 1e-3),)))]


def geometry(d, h):
    """The padded geometry the float64 tile kernels run a network on (csrc/mi_ode_api.hip, pick_family): 16 x 16 only when BOTH fit."""
    assert 1 <= d <= 64 and 1 <= h <= 128
    return (16, 16) if d <= 16 and h <= 16 else (64, 128)


def saturated(d, h, seed=81, batch=33):
    """(weights, y0) that drive the first layer into every arm of the float64 activations: b1 = linspace(-800, 800, h) with eight entries
    replaced by +-0.0625 * (1 +- 1e-3) (the switch between tanh's polynomial and its exp form) and +-30 * (1 +- 1e-3) (softplus' guard); row 0
    of y0 is zero, so its layer-1 pre-activations ARE b1; the other rows are uniform in [-1, 1].  The ends of the linspace are beyond
    +-710, where exp overflows / underflows in float64."""
    assert h >= 16
    ws = make_net(d, h, seed)
    b1 = np.linspace(-800., 800., h)
    edges = [s_ * v * (1 + e) for v in (0.0625, 30.0) for s_ in (-1, 1) for e in (-1e-3, 1e-3)]
    lo = h // 2 - 4
    b1[lo:lo + 8] = edges
    ws[1] = b1
    y0 = np.random.default_rng(seed + 1000).uniform(-1., 1., (batch, d))
    y0[0] = 0.0
    return ws, y0


STATUS = Case('status', 64, 128, 'tanh', 'dopri5', T_FWD, 65, seed=11, **REJ)
HANDLE = Case('handle', 6, 16, 'tanh', 'dopri5', T_FWD, 33, seed=71, gain=2.0)

ADAPTIVE_CASES = list(dict.fromkeys(MULTI_ADAPTIVE + WIDTH_EDGES + SCHEDULES + DENSE + [STATUS, HANDLE]))
ALL_CASES = {c.name: c for c in ADAPTIVE_CASES + MULTI_FIXED + FIXED_OPTIONS}


def ids(cases):
    return [c.name for c in cases]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle, once per (case, batch)
# ---------------------------------------------------------------------------------------------------------------------------------------
def inputs(case, cus=DEFAULT_CUS, batch=None):
    """(weights, f, y0, t) of a case in numpy."""
    ws = make_net(case.d, case.h, case.seed, case.td, case.bias, case.gain)
    return ws, np_f(ws, case.act, case.td), make_y0(batch_of(case, cus) if batch is None else batch, case.d, case.seed, case.spread), np.array(case.t)


@contextlib.contextmanager
def _recorded_ratios(O, out):
    """Every attempt's mean error ratio, as the oracle's controller receives it (the number `ratio <= 1` accepts on)."""
    a, b = O.optimal_step_size, O.optimal_step_size_tsit5

    def misc(last_step, ratios, *args, **kw):
        out.append(float(max(ratios)))
        return a(last_step, ratios, *args, **kw)

    def tsit5(last_step, ratio, *args, **kw):
        out.append(float(ratio))
        return b(last_step, ratio, *args, **kw)
    O.optimal_step_size, O.optimal_step_size_tsit5 = misc, tsit5
    try:
        yield
    finally:
        O.optimal_step_size, O.optimal_step_size_tsit5 = a, b


def oracle_options(case):
    opts = dict(case.options or ())
    if case.method == 'tsit5':
        opts['tsit5_fixed'] = True                     # the product integrates with Tsitouras' published error weights
    if case.first_step is not None:
        opts['first_step'] = case.first_step
    return opts or None


@functools.lru_cache(maxsize=None)
def _oracle(case, batch):
    from oracle import ode_numpy as O
    _, f, y0, t = inputs(case, batch=batch)
    ratios = []
    with _recorded_ratios(O, ratios):
        ref, st = O.odeint(f, y0, t, rtol=case.rtol, atol=case.atol, method=case.method, options=oracle_options(case), return_stats=True)
    ref.setflags(write=False)
    return ref, st, tuple(ratios)


def oracle(case, cus=DEFAULT_CUS, batch=None):
    """(solution [T, batch, d] (read only), oracle Stats, the attempts' error ratios) - computed once per process."""
    return _oracle(case, batch_of(case, cus) if batch is None else batch)


def steps_with_outputs(case, stats):
    """Per accepted step of an oracle run: how many requested output times fall in (t0, t0 + dt]."""
    sign = -1.0 if case.t[-1] < case.t[0] else 1.0
    t = sign * np.array(case.t[1:])
    return [int(np.sum((t > t0) & (t <= t0 + dt))) for t0, dt, acc, _ in stats.trace if acc]
