"""Shared inputs of the edge tests of the fused convolutional stage kernel (csrc/mi_ode_conv.h, k_conv_stage<T, ACT, TD>; host side
csrc/mi_ode_conv.hip, rhs.Conv2dODE, Conv2dODEFunc.device_rhs): the cases as data, their inputs and the oracle runs the GPU tests
(tests/test_gpu_conv_edges.py) compare with.  tests/test_conv_cases_host.py checks on the CPU that the cases have the properties the GPU
tests rely on, so that a GPU failure cannot be blamed on the inputs.  Nothing here needs a GPU.

The kernel: a 256-thread workgroup per 8 x 8 pixel tile of one image (tiles clip at the border), h1 on the tile plus a one-pixel halo,
conv2 as an MFMA GEMM over Fp = F padded to 16 in NB = Fp / 16 accumulator blocks, s_y with a stride of 16 channels.  What the cases are
chosen for: F on both sides of a block (1, 15, 16, 17), several blocks with a single live column in the last (113) and the full width (128:
no padding column, 116 KB of LDS in float64); C up to the stride of s_y (16); images of one pixel, one tile exactly, a one-pixel last tile
in one direction or both, one-pixel-high and -wide images with two tiles; batches up to 257 workgroups x tiles.

Inputs: the weights are a seeded models.Conv2dODEFunc's, times `scale` (2 in the existing conv tests), conv2's times `w2scale` on top;
y = yscale N(0, 1).  A float32 case's inputs are rounded to float32 and its comparison target is the float64 restatement on those rounded
inputs; its bound is 4 x max(E32, bands.case_ceiling(attempts, stages)) on |got - ref| / (1 + |ref|), with E32 the float32 restatement's
(or float32 oracle run's) own deviation from that target.  Nothing observed from the kernel enters a bound."""
import collections
import functools

import numpy as np
import torch

from oracle import ode_numpy as O
from tests import bands
from tests import conv_restatement as CR
from tests.mlp64_cases import _recorded_ratios, oracle_options

TILE = 8
ACTS = ('relu', 'softplus', 'tanh')
DTYPES = ('float64', 'float32')
F_CLASSES = (1, 15, 16, 17, 64, 113, 128)
C_CLASSES = (1, 2, 15, 16)
IMAGES = ((1, 1), (1, 9), (9, 1), (8, 8), (8, 9), (9, 8), (16, 16), (17, 17), (7, 23))
BATCHES = (1, 3, 257)
TIMES = (0.7, -1.3)                                      # the two evaluation times (opposite signs)
INSTANTIATIONS = tuple((d, a, td) for d in DTYPES for a in ACTS for td in (False, True))
F64_BAR = 1e-12                                         # max |got - ref| / max(1, max |ref|): the bar of tests/test_gpu_conv_odenet.py

_Eval = collections.namedtuple('Eval', 'name dtype act td B C H W F seed scale w2scale yscale')


def Eval(dtype, act, td, B, C, H, W, F, seed=0, scale=2.0, w2scale=1.0, yscale=1.0, prefix='eval'):
    name = '%s-%s-%s-%s-B%d-C%d-%dx%d-F%d' % (prefix, dtype, act, 'td' if td else 'ti', B, C, H, W, F)
    return _Eval(name, dtype, act, bool(td), B, C, H, W, F, seed, float(scale), float(w2scale), float(yscale))


def n_tiles(H, W):
    return (-(-H // TILE)) * (-(-W // TILE))


def n_blocks(F):
    """NB: the 16-column accumulator blocks of conv2."""
    return (F + 15) // 16


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _module_state(C, F, td, act, seed, scale, w2scale, dtype):
    from tfdiffeq_amd import models
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        fn = models.Conv2dODEFunc(C, F, time_dependent=td, non_linearity=act).double()
    with torch.no_grad():
        for p in fn.parameters():
            p.mul_(scale)
        fn.conv2.weight.mul_(w2scale)
        if dtype == 'float32':                          # the float64 inputs ARE the float32 inputs
            for p in fn.parameters():
                p.copy_(p.float().double())
    return {k: v.clone() for k, v in fn.state_dict().items()}


def module(case):
    """A fresh float64 CPU models.Conv2dODEFunc with the case's weights (rounded to float32 in a float32 case)."""
    from tfdiffeq_amd import models
    fn = models.Conv2dODEFunc(case.C, case.F, time_dependent=case.td, non_linearity=case.act).double()
    fn.load_state_dict(_module_state(case.C, case.F, case.td, case.act, case.seed, case.scale, case.w2scale, case.dtype))
    return fn


@functools.lru_cache(maxsize=None)
def params(case):
    return tuple((W, b) for W, b in CR.params(module(case)))


@functools.lru_cache(maxsize=None)
def state(case):
    """y [B, C, H, W] in float64 (float32-rounded in a float32 case), read only."""
    rng = np.random.default_rng(1000 * case.seed + 31 * case.C + 7 * case.F + case.H * case.W)
    y = case.yscale * rng.standard_normal((case.B, case.C, case.H, case.W))
    if case.dtype == 'float32':
        y = y.astype(np.float32).astype(np.float64)
    y.setflags(write=False)
    return y


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(case, t):
    """The float64 restatement at time t: the comparison target (read only, once per process)."""
    return _ro(CR.f(list(params(case)), t, state(case), case.act, case.td))


@functools.lru_cache(maxsize=None)
def e32(case, t):
    """E32: the float32 restatement's own deviation from `reference` in the measure of the float32 bar."""
    with np.errstate(over='ignore'):
        return bands.observed(CR.f32(list(params(case)), t, state(case), case.act, case.td), reference(case, t))


def f32_bound(case, t):
    return 4.0 * max(e32(case, t), bands.case_ceiling(1, stages=3))


def defects_of(case):
    return tuple(d for d in CR.DEFECTS if case.td or d != 'time_taps_unclipped')


def power(case, t):
    """{defect: the deviation of the float64 restatement with that defect from the right one, in the measure of the float32 bar}."""
    return {d: bands.observed(CR.f(list(params(case)), t, state(case), case.act, case.td, defect=d), reference(case, t)) for d in defects_of(case)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# evaluation cases: every instantiation sees every image class and every F class; C and the batch rotate with them
# ---------------------------------------------------------------------------------------------------------------------------------------
# (seed, scale, ...) of the cases whose default inputs missed max |ref| >= 0.3 or the power threshold (tests/test_conv_cases_host.py)
#   relu at F = 1: seed 0's single filter is dead on these inputs (the output is b3 everywhere and no defect can show)
TWEAKS = {'eval-float64-relu-ti-B257-C1-1x1-F1': dict(seed=6), 'eval-float32-relu-ti-B1-C2-7x23-F1': dict(seed=2)}


def _batch(i, q, H, W, F):
    if (H, W) == (1, 1):
        return 257
    if (H, W) == (8, 8):
        return 257 if F < 113 else 3
    b = 3 if (i + q) % 2 else 1
    return 1 if (F >= 113 and b * H * W > 600) else b


def _eval_cases():
    out = []
    for q, (dtype, act, td) in enumerate(INSTANTIATIONS):
        for i, (H, W) in enumerate(IMAGES):
            F = F_CLASSES[(i + q) % len(F_CLASSES)]
            C = C_CLASSES[(i + q // 2 + i // 4) % len(C_CLASSES)]
            c = Eval(dtype, act, td, _batch(i, q, H, W, F), C, H, W, F)
            out.append(c._replace(**TWEAKS.get(c.name, {})))
    return out


EVAL = _eval_cases()
# row independence (f(y)[i] against f(y[i:i+1])) and repeatability: several tiles, a batch of three, both dtypes
BATCH_ROWS = [c for c in EVAL if c.B == 3 and n_tiles(c.H, c.W) >= 2 and c.act == 'tanh']

# ---------------------------------------------------------------------------------------------------------------------------------------
# saturation: at least 1 % of the conv1 and of the conv2 pre-activations above 20 and at least 1 % below -20 (softplus's threshold;
# tanh is +-1 to the last bit long before)
# ---------------------------------------------------------------------------------------------------------------------------------------
SATURATED = [Eval(dtype, act, td, 3, 3, 9, 9, 17, seed=5, scale=2.0, w2scale=w2, yscale=40.0, prefix='sat')
             for dtype in DTYPES for act, w2 in (('softplus', 1.0), ('tanh', 40.0)) for td in (False, True)]


def pre_activations(case, t):
    """(z1, z2): what conv1 and conv2 hand to the activation in the float64 restatement."""
    p = params(case)

    def cat(x):
        return np.concatenate([np.full_like(x[:, :1], float(t)), x], axis=1) if case.td else x
    z1 = CR.conv2d(cat(state(case)), p[0][0], p[0][1], 0)
    z2 = CR.conv2d(cat(CR.act(case.act, z1)), p[1][0], p[1][1], 1)
    return z1, z2


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage(): 17 x 9 (3 x 2 tiles, a one-pixel last row of tiles), three images
# ---------------------------------------------------------------------------------------------------------------------------------------
STAGE = {dtype: Eval(dtype, 'tanh', True, 3, 5, 17, 9, 17, seed=2, prefix='stage') for dtype in DTYPES}
STAGE_NK = (0, 1, 7, 14)
# non-finite values: 17 x 17, three images, one pixel at the tile corner (7, 7) of the middle one
NONFINITE = [Eval(dtype, act, True, 3, 2, 17, 17, 17, seed=3, prefix='nonfinite') for dtype in DTYPES for act in ACTS]
NONFINITE_AT = (1, 0, 7, 7)                               # (image, channel, y, x)
# dtype crossing and stale weights
CROSSING = Eval('float64', 'softplus', True, 2, 3, 9, 9, 17, seed=4, prefix='crossing')


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole solves on the numpy oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
_Solve = collections.namedtuple('Solve', 'name dtype method act td B C H W F seed scale w2scale yscale t rtol atol rejecting first_step options')
STAGES = {'dopri5': 7, 'tsit5': 7, 'bosh3': 4, 'adaptive_heun': 2, 'dopri8': 13}


def Solve(dtype, method, act, td, t, B=2, C=3, H=9, W=7, F=10, seed=1, scale=2.0, yscale=0.5, rtol=1e-7, atol=1e-9, rejecting='', tag='', first_step=None):
    name = 'solve-%s-%s-%s-%s-%s%s' % (dtype, method, act, 'td' if td else 'ti', 'up' if t[-1] > t[0] else 'down', tag)
    return _Solve(name, dtype, method, act, bool(td), B, C, H, W, F, seed, float(scale), 1.0, float(yscale), tuple(float(v) for v in t), rtol, atol, rejecting, first_step, None)


UP, DOWN = (0.0, 0.5, 1.0), (1.0, 0.5, 0.0)
SOLVES = [
    Solve('float64', 'dopri5', 'softplus', True, UP, F=17),
    Solve('float64', 'dopri5', 'tanh', False, DOWN),
    Solve('float64', 'dopri5', 'relu', True, UP, F=17, tag='-relu'),
    Solve('float64', 'tsit5', 'tanh', True, DOWN, F=17),
    Solve('float64', 'bosh3', 'softplus', False, UP, rtol=1e-5, atol=1e-7),
    Solve('float64', 'adaptive_heun', 'tanh', True, UP, rtol=1e-4, atol=1e-6),
    Solve('float64', 'dopri8', 'softplus', True, DOWN, F=17),
    Solve('float32', 'dopri5', 'tanh', True, UP, F=17, scale=3.0, yscale=2.0, rtol=1e-4, atol=1e-5),
    Solve('float32', 'dopri5', 'softplus', False, DOWN, scale=2.0, yscale=1.0, rtol=1e-4, atol=1e-5),
    Solve('float32', 'dopri8', 'tanh', False, UP, scale=3.0, yscale=2.0, rtol=1e-4, atol=1e-5),
]
# scaled until the oracle rejects attempts: the FSAL last stage of a rejected attempt has written y_out, and the next attempt starts from
# the old state.  'first': the first attempt is rejected (a first_step of half the interval, which the oracle and the solver
# both take); 'after': a rejection after accepted steps (one case: two in a row); 'covered': a REJECTED attempt whose span holds the interior
# output time.  (The tsit5 case of SOLVES rejects attempts too, at its plain scale.)
REJECTING = [
    Solve('float64', 'dopri5', 'tanh', True, UP, F=17, scale=4.0, yscale=4.0, seed=3, first_step=0.5, rejecting='first after', tag='-rej-first'),
    Solve('float64', 'dopri5', 'tanh', True, UP, F=17, scale=4.0, yscale=8.0, rejecting='after', tag='-rej-after'),
    Solve('float64', 'dopri5', 'tanh', True, UP, F=17, scale=4.0, yscale=4.0, rejecting='after covered', tag='-rej-covered'),
]
ALL_SOLVES = SOLVES + REJECTING

Run = collections.namedtuple('Run', 'sol n_attempts n_accepted trace ratios')


def run_solve(case, dtype):
    """The oracle's solve of a case with the restatement as the right-hand side, in `dtype`; ratios: every attempt's largest error ratio as the
    controller receives it (tsit5: its pooled mean)."""
    p = CR.params(module(case))
    y0 = solve_state(case).astype(np.dtype(dtype))
    rhs = (lambda t_, y_: CR.f(p, t_, y_, case.act, case.td)) if dtype == 'float64' else (lambda t_, y_: CR.f32(p, t_, y_, case.act, case.td))
    ratios = []
    with _recorded_ratios(O, ratios):                    # (tsit5 with Tsitouras' published error weights, as the product: mlp64_cases.oracle_options)
        sol, st = O.odeint(rhs, y0, np.array(case.t), rtol=case.rtol, atol=case.atol, method=case.method, options=oracle_options(case), return_stats=True)
    return Run(_ro(np.asarray(sol)), st.n_attempts, st.n_accepted, tuple(st.trace), tuple(ratios))


def solve_state(case):
    rng = np.random.default_rng(77 * case.seed + case.F)
    y = case.yscale * rng.standard_normal((case.B, case.C, case.H, case.W))
    return y.astype(np.float32).astype(np.float64) if case.dtype == 'float32' else y


@functools.lru_cache(maxsize=None)
def oracle(case, dtype='float64'):
    """The oracle Run of a solve case (read only, once per process).  'float64' on a float32 case: the run on the rounded inputs, the target."""
    return run_solve(case, dtype)


def accepts(run):
    return ''.join('A' if row[2] else 'r' for row in run.trace)


def solve_e32(case):
    return bands.observed(oracle(case, 'float32').sol, oracle(case, 'float64').sol)


def solve_bound(case):
    return 4.0 * max(solve_e32(case), bands.case_ceiling(oracle(case, 'float32').n_attempts, stages=STAGES[case.method]))


def ids(cases):
    return [c.name for c in cases]
