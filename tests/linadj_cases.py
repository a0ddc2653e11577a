"""Shared inputs of the edge tests of the one-launch linear adjoint kernel (csrc/mi_ode_linadj.h, k_linadj<T, D>): the cases as data, their
inputs in numpy and the oracle runs the GPU tests (tests/test_gpu_linadj_edges.py) compare with.  tests/test_linadj_cases_host.py checks on the
CPU that the cases have the properties the GPU tests rely on - rejected attempts where a case is marked rejecting, a finite first guess h0 of
the initial step where it is marked so, 60 accepted steps of the long case, equal attempt counts of the float32 and the float64 oracle runs,
the intended grid and last-tile row count of every batch - so that a GPU failure cannot be blamed on the inputs.  Nothing here needs a GPU.

The oracle is oracle/ode_numpy.odeint over the tuple (y, adj_y, adj_t, adj_params) with the augmented dynamics of adjoint.py:69-105 restated
for f = y W + b, exactly as tests/test_gpu_linadj.py builds it.

Matrix families:
  base   -0.4 I + 0.6 (S - S^T) / sqrt(dim) + 0.1 R / sqrt(dim)      (tests/test_gpu_linadj.py's)
  rot    6 (S - S^T) / sqrt(dim)                                      rotation dominated: many accepted steps, nothing decays
  stiff  Q diag(-logspace(lo, hi, dim)) Q^T                           symmetric, log-spaced eigenvalues up to 1e3 over a short interval: the
                                                                      first step is too long (rejected two or three times) and one more
                                                                      attempt is rejected after accepted steps; max |adj_params| < 20

Batches that depend on the device are functions of its compute-unit count: the kernel's grid is G = min(ceil(batch / 16), CUs) workgroups.
('G', n): 16 n - 5 rows - n tiles, the last with 11 rows; 'CUS' / 'CUS-1': ('G', CUs) / ('G', CUs - 1); 'FULL': 16 CUs + 11 rows - every
workgroup one tile and 0 a second one, of 11 rows.

Float32 cases: the kernel carries adj_params in float64 where the oracle carries it in float32, so the comparison target is the float64 oracle
run on the float32-rounded inputs; the bound of a case is 4 x max(E32, bands.case_ceiling(n_attempts)) with E32 the float32 oracle run's own
deviation from that target (f32_bound)."""
import collections
import functools

import numpy as np

from tests import bands

DEFAULT_CUS = 256
TILE = 16
MAX_G = 256                                             # kLaMaxG

_Case = collections.namedtuple('Case', 'name family dim batch bias dtype t0 t1 rtol atol seed grad adjt spec rejecting finite_h0 th0')


def Case(name, dim, batch, t0, t1, family='base', bias=True, dtype='float64', rtol=None, atol=None, seed=1, grad=True, adjt=0.37, spec=None,
         rejecting=False, finite_h0=False, th0=0.01):
    if rtol is None:
        rtol, atol = (1e-7, 1e-10) if dtype == 'float64' else (1e-4, 1e-5)
    return _Case(name, family, dim, batch, bias, dtype, float(t0), float(t1), rtol, atol, seed, grad, adjt, spec, rejecting, finite_h0, th0)


def batch_of(case_or_batch, cus=DEFAULT_CUS):
    b = case_or_batch.batch if isinstance(case_or_batch, _Case) else case_or_batch
    if b == 'FULL':
        return TILE * cus + 11
    if b == 'CUS':
        b = ('G', cus)
    elif b == 'CUS-1':
        b = ('G', cus - 1)
    return TILE * b[1] - 5 if isinstance(b, tuple) else int(b)


def n_tiles(batch):
    return -(-batch // TILE)


def grid_of(batch, cus=DEFAULT_CUS):
    """G of mi_ode_linadj_create: every workgroup co-resident, at most one per compute unit."""
    return max(1, min(n_tiles(batch), cus, MAX_G))


def last_tile_rows(batch):
    return batch - TILE * (n_tiles(batch) - 1)


def tile_width(dim):
    """la_pad_dim: the D of the k_linadj<T, D> a dim runs on."""
    return 16 if dim <= 16 else 32 if dim <= 32 else 64 if dim <= 64 else 128


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def matrix(family, dim, rng, spec=None):
    S = rng.standard_normal((dim, dim))
    if family == 'base':
        return -0.4 * np.eye(dim) + 0.6 * (S - S.T) / np.sqrt(dim) + 0.1 * rng.standard_normal((dim, dim)) / np.sqrt(dim)
    if family == 'rot':
        return 6.0 * (S - S.T) / np.sqrt(dim)
    if family == 'stiff':
        lo, hi = spec
        Q, _ = np.linalg.qr(S)
        return (Q * -np.logspace(lo, hi, dim)) @ Q.T
    raise KeyError(family)


Inputs = collections.namedtuple('Inputs', 'W b y a g adjt th')


def inputs(case, cus=DEFAULT_CUS, dtype=None):
    """The inputs of one segment call in numpy: float64 values, rounded to the case's dtype and returned in `dtype` (default: the case's) -
    so a float32 case's float64 inputs ARE its float32 inputs."""
    batch, dim = batch_of(case, cus), case.dim
    rng = np.random.default_rng(1000 * case.seed + dim)
    W = matrix(case.family, dim, rng, case.spec)
    b = 0.3 * rng.standard_normal(dim) if case.bias else None
    y = rng.standard_normal((batch, dim))
    a = rng.standard_normal((batch, dim)) / batch
    g = rng.standard_normal((batch, dim)) / batch if case.grad else None      # grad_output at t0: the time gradient's dot product
    adjt = np.array(case.adjt)
    th = case.th0 * rng.standard_normal(dim * dim + (dim if case.bias else 0))
    own = np.dtype(case.dtype)
    out = np.dtype(dtype or case.dtype)
    return Inputs(*(None if v is None else v.astype(own).astype(out) for v in (W, b, y, a, g, adjt, th)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple('Result', 'adj_y adj_t adj_params dldt n_attempts n_accepted h0 trace ratios')


def augmented(W, b):
    """adjoint.py:69-105 for f = y W + b."""
    def aug(t_, s_):
        y_, a_ = s_[0], s_[1]
        f = y_ @ W + (b if b is not None else 0.0)
        vth = -(y_.T @ a_).reshape(-1)
        if b is not None:
            vth = np.concatenate([vth, -a_.sum(0)])
        return (f, -(a_ @ W.T), np.zeros_like(s_[2]), vth)
    return aug


def first_guess_h0(aug, t0, state, rtol, atol):
    """h0 of misc.py:225-233 with the oracle's own norms (oracle/ode_numpy.select_initial_step computes it and returns min(100 h0, h1)):
    +inf when a component has d1 = 0 and d0 > 0 - adj_t, whose derivative is zero, unless adj_t itself is zero."""
    from oracle import ode_numpy as O
    dtype = state[0].dtype
    f0 = aug(O._scalar(t0, dtype), state)
    with np.errstate(all='ignore'):
        scale = tuple((atol + np.abs(v) * rtol).astype(dtype) for v in state)
        d0 = tuple(O._rms_norm(v / s) for v, s in zip(state, scale))
        d1 = tuple(O._rms_norm(f / s) for f, s in zip(f0, scale))
        if O._pymax(d0) < 1e-5 or O._pymax(d1) < 1e-5:
            return float(O._scalar(1e-6, dtype))
        return float(0.01 * O._pymax([p / q for p, q in zip(d0, d1)]))


def theta_decides_first_step(case, cus=DEFAULT_CUS):
    """(the first step size of the tuple system, the same with the adj_params component's derivative left out of the initial step's norms)
    by the oracle's select_initial_step: unequal when adj_params decides."""
    from oracle import ode_numpy as O
    x = inputs(case, cus, 'float64')
    sgn = -1.0 if case.t1 < case.t0 else 1.0
    aug = augmented(x.W, x.b)
    state = (x.y, x.a, x.adjt, x.th)
    full = lambda t_, s_: tuple(sgn * v for v in aug(t_, s_))  # noqa: E731
    without = lambda t_, s_: full(t_, s_)[:3] + (np.zeros_like(s_[3]),)  # noqa: E731
    return tuple(float(O.select_initial_step(f, sgn * case.t0, state, 4, case.rtol, case.atol)[0]) for f in (full, without))


def run_oracle(x, t0, t1, rtol, atol):
    """One backward interval t0 -> t1 of the tuple system on the inputs `x`, in their dtype."""
    from oracle import ode_numpy as O
    aug = augmented(x.W, x.b)
    if x.g is not None:
        dl = ((x.y @ x.W + (x.b if x.b is not None else 0.0)) * x.g).sum()          # adjoint.py:134-140
        adjt0 = (x.adjt - dl).astype(x.y.dtype)
    else:
        dl, adjt0 = 0.0, x.adjt
    state = (x.y, x.a, adjt0, x.th)
    ratios, step_size = [], O.optimal_step_size

    def recording(last_step, rs, *args, **kw):              # every attempt's largest error ratio, as the oracle's controller receives it
        ratios.append(float(max(rs)))
        return step_size(last_step, rs, *args, **kw)
    O.optimal_step_size = recording
    try:
        sol, st = O.odeint(aug, state, np.array([t0, t1]), rtol=rtol, atol=atol, method='dopri5', return_stats=True)
    finally:
        O.optimal_step_size = step_size
    res = Result(np.asarray(sol[1][1]), np.asarray(sol[2][1]), np.asarray(sol[3][1]), float(dl), st.n_attempts, st.n_accepted,
                 first_guess_h0(aug, t0, state, rtol, atol), tuple(st.trace), tuple(ratios))
    for v in res[:3]:
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _oracle(case, cus, dtype):
    return run_oracle(inputs(case, cus, dtype), case.t0, case.t1, case.rtol, case.atol)


def oracle(case, cus=DEFAULT_CUS, dtype='float64'):
    """The oracle's Result of a case (read only, once per process).  dtype 'float64' on a float32 case: the float64 run on the float32-rounded
    inputs, the comparison target of the float32 kernels."""
    return _oracle(case, cus, dtype)


def f32_error(case, cus=DEFAULT_CUS):
    """E32: the float32 oracle run's deviation from the float64 run on the same inputs (bands.observed, worst of the three outputs)."""
    lo, hi = oracle(case, cus, 'float32'), oracle(case, cus, 'float64')
    return max(bands.observed(p, q) for p, q in zip(lo[:3], hi[:3]))


def f32_bound(case, cus=DEFAULT_CUS):
    """4 x max(E32, the project's a-priori float32 ceiling for that many attempts); 4: the slab product's different summation order, a
    sqrt(batch)-ulp effect at these batches."""
    assert case.dtype == 'float32'
    return 4.0 * max(f32_error(case, cus), bands.case_ceiling(oracle(case, cus, 'float32').n_attempts))


F64_BAR = 1e-11                                         # |got - ref| <= F64_BAR * max(1, max |ref|): the project's bar for this kernel


def carried_g0_drift(case, cus=DEFAULT_CUS):
    """The relative drift of G0 | g0 carried from step to step in the power form (oracle/linear_adjoint_numpy.end_state_products_powers chained
    over the oracle's accepted step sizes) against y^T a | sum_rows a of the oracle's own states after the same steps (its Runge-Kutta step
    applied to (y, a) with those step sizes): worst step, max |difference| / max |product|."""
    from oracle import linear_adjoint_numpy as LA
    from oracle import ode_numpy as O
    x = inputs(case, cus, 'float64')
    s = -1.0 if case.t1 < case.t0 else 1.0
    fy = (lambda t_, y_: (s * (y_[0] @ x.W + x.b),)) if x.b is not None else (lambda t_, y_: (s * (y_[0] @ x.W),))
    fa = lambda t_, a_: (-s * (a_[0] @ x.W.T),)  # noqa: E731
    y, a = (x.y,), (x.a,)
    ky, ka = fy(0.0, y), fa(0.0, a)
    G, g = x.y.T @ x.a, x.a.sum(0)
    worst = 0.0
    for t_, dt, accepted, _ in oracle(case, cus).trace:
        if not accepted:
            continue
        y, ky, _, _ = O.runge_kutta_step(fy, y, ky, t_, dt, O.DOPRI5)
        a, ka, _, _ = O.runge_kutta_step(fa, a, ka, t_, dt, O.DOPRI5)
        G, g = LA.end_state_products_powers(x.W, x.b, G, g, dt, s, O.DOPRI5)
        Gs, gs = y[0].T @ a[0], a[0].sum(0)
        worst = max(worst, float(np.abs(G - Gs).max() / np.abs(Gs).max()), float(np.abs(g - gs).max() / np.abs(gs).max()))
    return worst


def long_bound(case, cus=DEFAULT_CUS):
    """max(1e-11, 10 x the reference's own drift of the carried G0); 10: the kernel's different summation order in its D x D products."""
    return max(F64_BAR, 10.0 * carried_g0_drift(case, cus))


def bound_of(case, cus=DEFAULT_CUS):
    if case.dtype == 'float32':
        return f32_bound(case, cus)
    return long_bound(case, cus) if case is LONG else F64_BAR


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
BOXES = {16: (1, 3, 16), 32: (17, 20, 32), 64: (33, 48, 64), 128: (65, 127, 128)}
DOWN, UP = (1.0, 0.0), (0.0, 0.8)

# a. every instantiation: batch 100 (7 tiles, the last with 4 rows); per tile width the middle dim runs in increasing time
EVERY = [Case('%s-d%d-%s' % (dt[5:], dim, 'b' if bias else 'nb'), dim, 100, *(UP if i == 1 else DOWN), bias=bias, dtype=dt, seed=11 + i)
         for dt in ('float64', 'float32') for width in (16, 32, 64, 128) for i, dim in enumerate(BOXES[width]) for bias in (True, False)]
TINY = [Case('%s-d%d-B%d' % (dt[5:], dim, batch), dim, batch, *DOWN, dtype=dt, seed=17)
        for dt in ('float64', 'float32') for dim in (3, 128) for batch in (1, 15)]

# b. natural grids
GRIDS = ([Case('grid-d20-G%s' % (g if isinstance(g, str) else g[1]), 20, g, *DOWN, seed=21)
          for g in [('G', n) for n in (1, 2, 7, 8, 49, 50, 56, 57, 105)] + ['CUS-1', 'CUS']] +
         [Case('grid-d128-G%s' % (g if isinstance(g, str) else g[1]), 128, g, *DOWN, seed=22) for g in (('G', 1), ('G', 2), ('G', 50), 'CUS')] +
         [Case('grid-d5-GCUS', 5, 'CUS', *DOWN, seed=23), Case('grid-d16-GCUS', 16, 'CUS', *UP, bias=False, seed=24),
          Case('grid-32-d20-GCUS', 20, 'CUS', *DOWN, dtype='float32', seed=25)])

# c. grids by override: batch 369 = 24 tiles, the last with one row
OVERRIDE_GRIDS = (1, 2, 5, 24)
OVERRIDE = [Case('override-d20', 20, 369, *DOWN, seed=31), Case('override-d100', 100, 369, *UP, bias=False, seed=32)]

# d. rejected attempts: the stiff family - the spectrum and the interval chosen so that max |adj_params(t_end)| stays below 1e3
_REJ = dict(family='stiff', rejecting=True)
_T6 = dict(rtol=1e-6, atol=1e-9)
REJECTING = [
    Case('rej-d12', 12, 300, 0.012, 0.0, spec=(-1.0, 3.0), seed=41, **_REJ, **_T6),
    Case('rej-d24', 24, 300, 0.0, 0.03, spec=(0.0, 2.6), seed=42, **_REJ, **_T6),
    Case('rej-d40', 40, 300, 0.0, 0.012, spec=(-1.0, 3.0), bias=False, seed=47, **_REJ, **_T6),
    Case('rej-d100', 100, 300, 0.012, 0.0, spec=(0.0, 3.0), seed=44, **_REJ, **_T6),
    Case('rej-32-d24', 24, 300, 0.0, 0.012, spec=(-1.0, 3.0), dtype='float32', seed=45, **_REJ),
    Case('rej-full-d24', 24, 'FULL', 0.012, 0.0, spec=(-1.0, 3.0), seed=46, **_REJ, **_T6),
]

# e. adj_t = 0 at the interval's start and no grad_out: the first guess h0 of the initial step is finite
FINITE_H0 = [Case('h0-d%d-%s' % (dim, 'b' if bias else 'nb'), dim, 200, *(DOWN if bias else UP), bias=bias, grad=False, adjt=0.0, seed=51, finite_h0=True)
             for dim in (5, 20, 128) for bias in (True, False)]

# ... and with adj_params = 0 at the start on the rotation family: its scale is atol alone and its second derivative large, so the adj_params
# share of the second evaluation (the m00 + sh m10 - sh m01 - sh^2 m11 combination) DECIDES the first step size (theta_decides_first_step)
FINITE_H0 += [Case('h0-theta-d%d' % dim, dim, 200, *d, family='rot', bias=bias, grad=False, adjt=0.0, th0=0.0, seed=52, finite_h0=True, rtol=1e-6, atol=1e-10)
              for dim, bias, d in ((20, True, (0.0, 0.3)), (100, False, (0.3, 0.0)))]

# f. a long interval
LONG = Case('long-rot-d24', 24, 200, 0.0, 2.0, family='rot', rtol=1e-6, atol=1e-9, seed=61)

# g. one handle, these in order (same batch, dim, dtype, tolerances)
HANDLE = [Case('handle-bias', 20, 250, *DOWN, seed=71), Case('handle-nobias', 20, 250, *DOWN, bias=False, seed=72),
          Case('handle-bias-other-w', 20, 250, *DOWN, seed=73), Case('handle-down', 20, 250, 0.9, 0.2, seed=74),
          Case('handle-up', 20, 250, *UP, seed=75)]

# h. status: a NaN in the ragged last tile, then the same engine on this clean case
STATUS = Case('status', 20, 100, *DOWN, seed=81)

SEGMENT_CASES = EVERY + TINY + GRIDS + OVERRIDE + REJECTING + FINITE_H0 + [LONG] + HANDLE + [STATUS]
ALL_CASES = {c.name: c for c in SEGMENT_CASES}
assert len(ALL_CASES) == len(SEGMENT_CASES)


def ids(cases):
    return [c.name for c in cases]
