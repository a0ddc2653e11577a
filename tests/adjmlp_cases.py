"""Shared inputs of the edge tests of the fused MLP adjoint kernel (csrc/mi_ode_adjoint.h, k_adjoint_mlp<DP, HP, ACT, 6>): the cases as data,
their inputs in numpy and the oracle runs the GPU tests (tests/test_gpu_adjoint_fused_edges.py) compare with.
tests/test_adjmlp_cases_host.py checks on the CPU that the cases have the properties the GPU tests rely on - see `admission` - so that a GPU
failure cannot be blamed on the inputs.  Nothing here needs a GPU.

The oracle is oracle/ode_numpy.odeint (dopri5, scalar rtol / atol) over the tuple (y, adj_y, adj_t, adj_params) with the augmented dynamics
of adjoint.py:69-105 restated in numpy for the ODEFunc network dim -> hidden -> hidden -> dim (`augmented`): tanh, relu or softplus (beta 1,
threshold 20), time independent or time dependent (W1 = [1 + dim, hidden], row 0 = w_t, the row that multiplies t).  adj_params is in the
kernel's canonical order (w_t,) W1 b1 W2 b2 W3 b3 with [in, out] weights; adj_t's derivative is dot(w_t, -a^T df/db1).

Inputs: W = scale N(0, 1) / sqrt(fan_in), b = 0.1 N(0, 1), y = yscale N(0, 1), a = ascale N(0, 1) / batch, adj_params = th0 N(0, 1).  The scales are
large on purpose (tanh: 3 and 4): the augmented system then has a truncation error that steers the step size controller in float32 as it
does in float64.  On a mild problem the float32 error ratios are roundoff, the controller's choices differ between two float32
implementations, and no step-for-step comparison is possible.

Batches that depend on the device are functions of its compute-unit count: the kernel's grid is G = min(ceil(batch / 32), CUs) workgroups.
('G', n): 32 n - 21 rows - n tiles, the last with 11 rows; 'CUS' / 'CUS-1': ('G', CUs) / ('G', CUs - 1); 'FULL': 32 CUs + 11 rows - every
workgroup one tile and workgroup 0 a second one, of 11 rows; 'FULL3': 64 CUs + 1 rows - a third trip of workgroup 0, with a one-row tile.

The kernel is float32 only.  The comparison target is the float64 oracle run on the float32-rounded inputs; the bound of a case is
4 x max(E32, bands.case_ceiling(n_attempts)) on |got - ref| / (1 + |ref|), with E32 the float32 oracle run's own deviation from that target
(`bound_of`).  Nothing observed from the kernel enters it."""
import collections
import functools

import numpy as np

from tests import bands

DEFAULT_CUS = 256
TILE = 32
MAX_G = 1024                                            # (kPersistMaxGrid is far above any compute-unit count)

_Case = collections.namedtuple('Case', 'name dim hidden batch act td t0 t1 rtol atol seed scale yscale ascale adjt th0 rejecting finite_h0')


def Case(name, dim, hidden, batch, t0, t1, act='tanh', td=False, rtol=1e-5, atol=1e-6, seed=1, scale=3.0, yscale=4.0, ascale=1.0, adjt=0.3,
         th0=0.01, rejecting=False, finite_h0=False):
    return _Case(name, dim, hidden, batch, act, bool(td), float(t0), float(t1), rtol, atol, seed, float(scale), float(yscale), float(ascale), adjt,
                 th0, rejecting, finite_h0)


def batch_of(case_or_batch, cus=DEFAULT_CUS):
    b = case_or_batch.batch if isinstance(case_or_batch, _Case) else case_or_batch
    if b == 'FULL':
        return TILE * cus + 11
    if b == 'FULL3':
        return 2 * TILE * cus + 1
    if b == 'CUS':
        b = ('G', cus)
    elif b == 'CUS-1':
        b = ('G', cus - 1)
    return TILE * b[1] - 21 if isinstance(b, tuple) else int(b)


def n_tiles(batch):
    return -(-batch // TILE)


def grid_of(batch, cus=DEFAULT_CUS):
    """The grid of mi_ode_adjoint_create: every workgroup co-resident, at most one per compute unit."""
    return max(1, min(n_tiles(batch), cus, MAX_G))


def last_tile_rows(batch):
    return batch - TILE * (n_tiles(batch) - 1)


def kernel_of(dim, hidden):
    """(DP, HP) of the k_adjoint_mlp<DP, HP, ACT, 6> a network runs on (pad16 in mi_ode_adjoint_create)."""
    return (16 if dim <= 16 else 64, 16 if hidden <= 16 else 128)


def block_of(dim, hidden):
    """Threads per workgroup: 64 x AdjGeom<DP, HP>::NW - a wavefront per 16 hidden columns or per 16 x 16 block of a 32-row state tile,
    whichever is more.  blockDim / 128 thread groups share the fold of adj_slice, unrolled 8 ways: its boundary is G = 8 blockDim / 128."""
    dp, hp = kernel_of(dim, hidden)
    return 64 * max(hp // 16, 2 * dp // 16)


def n_params(dim, hidden, td):
    return (hidden if td else 0) + dim * hidden + hidden + hidden * hidden + hidden + hidden * dim + dim


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple('Inputs', 'W1 b1 W2 b2 W3 b3 y a adjt th')


def inputs(case, cus=DEFAULT_CUS, dtype='float32'):
    """The inputs of one segment call in numpy: generated in float64, rounded to float32 and returned in `dtype` - so the float64 inputs ARE
    the float32 inputs.  W1 is [td + dim, hidden]."""
    batch, dim, hd = batch_of(case, cus), case.dim, case.hidden
    rng = np.random.default_rng(1000 * case.seed + 7 * dim + hd)
    din = dim + (1 if case.td else 0)
    W1 = case.scale * rng.standard_normal((din, hd)) / np.sqrt(din)
    b1 = 0.1 * rng.standard_normal(hd)
    W2 = case.scale * rng.standard_normal((hd, hd)) / np.sqrt(hd)
    b2 = 0.1 * rng.standard_normal(hd)
    W3 = case.scale * rng.standard_normal((hd, dim)) / np.sqrt(hd)
    b3 = 0.1 * rng.standard_normal(dim)
    th = case.th0 * rng.standard_normal(n_params(dim, hd, case.td))
    y = case.yscale * rng.standard_normal((batch, dim))
    a = case.ascale * rng.standard_normal((batch, dim)) / batch
    adjt = np.array(case.adjt, dtype=np.float64)
    return Inputs(*(v.astype(np.float32).astype(np.dtype(dtype)) for v in (W1, b1, W2, b2, W3, b3, y, a, adjt, th)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the augmented dynamics
# ---------------------------------------------------------------------------------------------------------------------------------------
def _act(name, z):
    """(act(z), act'(z))"""
    if name == 'tanh':
        h = np.tanh(z)
        return h, 1 - h * h
    if name == 'relu':
        return np.maximum(z, 0), (z > 0).astype(z.dtype)
    if name == 'softplus':                              # torch.nn.Softplus(beta=1, threshold=20): the identity above the threshold
        big = z > 20
        zs = np.where(big, 0, z)
        return np.where(big, z, np.logaddexp(zs, 0).astype(z.dtype)), np.where(big, 1, 0.5 + 0.5 * np.tanh(0.5 * zs)).astype(z.dtype)
    raise KeyError(name)


def augmented(x, act, td):
    """adjoint.py:69-105 for the ODEFunc network: (f, -a^T df/dy, -a^T df/dt, -a^T df/dtheta)."""
    wt, W1y = (x.W1[0], x.W1[1:]) if td else (None, x.W1)

    def aug(t_, s_):
        y_, a_ = s_[0], s_[1]
        dt = y_.dtype
        z1 = y_ @ W1y + x.b1
        if td:
            z1 = z1 + dt.type(t_) * wt
        h1, d1 = _act(act, z1)
        h2, d2 = _act(act, h1 @ x.W2 + x.b2)
        f = h2 @ x.W3 + x.b3
        g3 = -a_
        g2 = (g3 @ x.W3.T) * d2
        g1 = (g2 @ x.W2.T) * d1
        db1 = g1.sum(0)
        parts = [dt.type(t_) * db1] if td else []        # (the input of w_t is t in every row)
        parts += [(y_.T @ g1).reshape(-1), db1, (h1.T @ g2).reshape(-1), g2.sum(0), (h2.T @ g3).reshape(-1), g3.sum(0)]
        vt = np.asarray(wt @ db1, dtype=dt) if td else np.zeros_like(s_[2])
        return (f, g1 @ W1y.T, vt, np.concatenate(parts).astype(dt))
    return aug


DYNAMICS_BAR = 3e-6                                     # max |got - ref| / max |ref| of one evaluation: the bar of tests/test_gpu_adjoint_fused.py


def dynamics_inputs(case, cus=DEFAULT_CUS, dtype='float32'):
    """The inputs of ONE evaluation of the augmented dynamics of a case's network shape: W = N(0, 1) / sqrt(fan_in), y and a = N(0, 1), as
    the evaluations of tests/test_gpu_adjoint_fused.py.  (Not the segment's: with its weights of scale 3 the tanh layers saturate, a^T df/dy
    is a sum of cancelling terms, and a plain float32 evaluation of the restatement is itself 2.7e-6 off the float64 one at (64, 16) - the
    bar would test float32, not the kernel.  `dynamics_f32_error` of these inputs stays below a quarter of the bar.)"""
    return inputs(case._replace(scale=1.0, yscale=1.0, ascale=float(batch_of(case, cus))), cus, dtype)


def dynamics_reference(case, cus=DEFAULT_CUS, dtype='float64'):
    """(f, -a^T df/dy, -a^T df/dt, -a^T df/dtheta) at t0 of the case on `dynamics_inputs`."""
    x = dynamics_inputs(case, cus, dtype)
    return augmented(x, case.act, case.td)(np.dtype(dtype).type(case.t0), (x.y, x.a, x.adjt, x.th))


def dynamics_f32_error(case, cus=DEFAULT_CUS):
    """The float32 restatement's own deviation from the float64 one in that evaluation, in the measure of the bar (f, vjp_y, vjp_params)."""
    lo, hi = dynamics_reference(case, cus, 'float32'), dynamics_reference(case, cus, 'float64')
    return max(float(np.abs(p.astype(np.float64) - q).max()) / max(float(np.abs(q).max()), 1e-30) for p, q in ((lo[0], hi[0]), (lo[1], hi[1]), (lo[3], hi[3])))


def first_guess_h0(aug, t0, state, rtol, atol):
    """h0 of misc.py:225-233 with the oracle's own norms: +inf when a component has d1 = 0 and d0 > 0 - adj_t of a time-independent network,
    whose derivative is zero, unless adj_t itself is zero."""
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


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple('Result', 'adj_y adj_t adj_params n_attempts n_accepted h0 trace ratios')


def run_oracle(x, act, td, t0, t1, rtol, atol):
    """One backward interval t0 -> t1 of the tuple system on the inputs `x`, in their dtype.  trace: the oracle's rows (t0, dt, accepted,
    dt_next) in solver time (negated when t1 < t0); ratios: every attempt's four error ratios as the controller receives them."""
    from oracle import ode_numpy as O
    aug = augmented(x, act, td)
    state = (x.y, x.a, x.adjt, x.th)
    ratios, step_size = [], O.optimal_step_size

    def recording(last_step, rs, *args, **kw):
        ratios.append(tuple(float(r) for r in rs))
        return step_size(last_step, rs, *args, **kw)
    O.optimal_step_size = recording
    try:
        sol, st = O.odeint(aug, state, np.array([t0, t1]), rtol=rtol, atol=atol, method='dopri5', return_stats=True)
    finally:
        O.optimal_step_size = step_size
    res = Result(np.asarray(sol[1][1]), np.asarray(sol[2][1]), np.asarray(sol[3][1]), st.n_attempts, st.n_accepted,
                 first_guess_h0(aug, t0, state, rtol, atol), tuple(st.trace), tuple(ratios))
    for v in res[:3]:
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _oracle(case, cus, dtype):
    return run_oracle(inputs(case, cus, dtype), case.act, case.td, case.t0, case.t1, case.rtol, case.atol)


def oracle(case, cus=DEFAULT_CUS, dtype='float64'):
    """The oracle's Result of a case (read only, once per process).  'float64': the run on the float32-rounded inputs, the comparison target."""
    return _oracle(case, cus, dtype)


def f32_error(case, cus=DEFAULT_CUS):
    """E32: the float32 oracle run's deviation from the float64 run on the same inputs (bands.observed, worst of the three outputs)."""
    lo, hi = oracle(case, cus, 'float32'), oracle(case, cus, 'float64')
    return max(bands.observed(p, q) for p, q in zip(lo[:3], hi[:3]))


def bound_of(case, cus=DEFAULT_CUS):
    """4 x max(E32, the project's a-priori float32 ceiling for that many attempts) - the project's rule for a float32 one-launch kernel against
    a float64 oracle (linadj_cases.f32_bound); 4: the device's different summation order (k-ordered MFMA chains, per-workgroup partials
    folded across the grid)."""
    return 4.0 * max(f32_error(case, cus), bands.case_ceiling(oracle(case, cus, 'float32').n_attempts))


def accepts(result):
    """'AArA..': the accept / reject sequence of a run."""
    return ''.join('A' if row[2] else 'r' for row in result.trace)


def admission(case, cus=DEFAULT_CUS):
    """The conditions under which a case may be compared step for step with a float32 device run, from the oracle alone; returns a dict of
    figures and the list of conditions that fail (empty: admitted).
      a  the float32 and the float64 run have identical accept / reject sequences
      b  every attempt's largest error ratio is farther than 0.02 from 1 in both precisions
      c  every attempt's dt_next of the float32 run is within 5 % of the float64 run's: truncation error steers the controller, not roundoff
      d  the second-to-last accepted step ends farther than 1e-3 |t1 - t0| from t_end: no step boundary that roundoff could push across it
      e  max |adj_params| <= 1e3, max |adj_y| <= 1e3
      f  the bound is finite and below 1e-3
      g  the gap of (b) is larger than the two runs' own relative disagreement about an attempt's largest ratio"""
    lo, hi = oracle(case, cus, 'float32'), oracle(case, cus, 'float64')
    fails = []
    fig = dict(seq32=accepts(lo), seq64=accepts(hi))
    if fig['seq32'] != fig['seq64']:
        fails.append('a')
    fig['gap'] = min(abs(max(r) - 1.0) for res in (lo, hi) for r in res.ratios)
    if not fig['gap'] > 0.02:
        fails.append('b')
    # g  (stricter than b, added after the first GPU run): that gap is also larger than the two runs' own disagreement about a ratio - the
    #    worst relative difference of their largest ratios over the attempts where that ratio is above 0.01.  A case where the float32 run's
    #    ratios are 14 % off the float64 run's cannot promise a third float32 implementation the same decision at a ratio of 1.05.
    fig['noise'] = max([abs(max(p) - max(q)) / max(q) for p, q in zip(lo.ratios, hi.ratios) if max(max(p), max(q)) > 0.01] + [0.0])
    if not fig['gap'] > fig['noise']:
        fails.append('g')
    if 'a' not in fails:
        fig['dt_next'] = max(abs(p[3] - q[3]) / abs(q[3]) for p, q in zip(lo.trace, hi.trace))
        if not fig['dt_next'] <= 0.05:
            fails.append('c')
    span, t_end = abs(case.t1 - case.t0), (-case.t1 if case.t1 < case.t0 else case.t1)
    fig['end_gap'] = float('inf')
    for res in (lo, hi):
        ends = [row[0] + row[1] for row in res.trace if row[2]]
        if len(ends) >= 2:
            fig['end_gap'] = min(fig['end_gap'], abs(ends[-2] - t_end) / span)
    if not fig['end_gap'] > 1e-3:
        fails.append('d')
    fig['max_theta'], fig['max_adj_y'] = float(np.abs(hi.adj_params).max()), float(np.abs(hi.adj_y).max())
    if not (all(np.isfinite(v).all() for v in hi[:3] + lo[:3]) and fig['max_theta'] <= 1e3 and fig['max_adj_y'] <= 1e3):
        fails.append('e')
    fig['e32'], fig['bound'] = f32_error(case, cus), bound_of(case, cus)
    if not (np.isfinite(fig['bound']) and 0.0 < fig['bound'] < 1e-3):
        fails.append('f')
    return fig, fails


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
BOXES = {(16, 16): ((1, 1), (3, 5), (16, 16)), (16, 128): ((1, 17), (16, 17), (9, 128)),
         (64, 16): ((17, 1), (17, 16), (64, 16)), (64, 128): ((17, 17), (33, 70), (64, 128))}
DOWN, UP = 'down', 'up'
# The unbounded activations need smaller weights and a shorter interval: with the tanh recipe the parameter gradient grows to 1e9 and the
# two precisions fork; relu's kinks cost a rejected attempt each, and the a-priori ceiling of the bound grows with the attempts.
ACT_KW = {'tanh': dict(), 'relu': dict(scale=1.0), 'softplus': dict(scale=2.0)}
INTERVAL = {('tanh', DOWN): (1.0, 0.0), ('tanh', UP): (0.0, 0.8), ('relu', DOWN): (1.0, 0.6), ('relu', UP): (0.0, 0.4),
            ('softplus', DOWN): (1.0, 0.6), ('softplus', UP): (0.0, 0.4)}


def _mk(prefix, dim, hidden, batch, d, act='tanh', td=False, **kw):
    """A case of the common recipe: d is DOWN or UP (the activation's interval) or a pair (t0, t1)."""
    name = '%s-d%d-h%d-%s-%s' % (prefix, dim, hidden, act, 'td' if td else 'ti')
    if isinstance(d, str):
        name, d = name + '-' + d, INTERVAL[act, d]
    kw = dict(ACT_KW[act], **kw)
    kw['seed'] = SEEDS.get(name, kw.get('seed', 1))
    kw.update(TWEAKS.get(name, {}))
    return Case(name, dim, hidden, batch, d[0], d[1], act=act, td=td, **kw)


# Seeds (and, where no seed of the common recipe was admissible, scales or intervals) found by a search on the CPU for inputs that pass
# `admission`; tests/test_adjmlp_cases_host.py holds every case to it.
SEEDS = {
    'every-d1-h1-tanh-ti-down': 5,
    'every-d1-h1-relu-td-up': 4,
    'every-d3-h5-softplus-ti-up': 3,
    'every-d16-h16-relu-ti-down': 2,
    'every-d1-h17-tanh-ti-down': 2,
    'every-d9-h128-softplus-td-down': 2,
    'every-d64-h16-relu-ti-down': 3,
    'every-d33-h70-softplus-ti-up': 2,
    'override-d10-h24-tanh-ti-down': 2,
    'rej-d8-h32-tanh-ti-down': 2,
    'rej-d64-h16-tanh-td-down': 8,
    'rej-d33-h70-tanh-td-down': 10,                      # (seed 1 is every-d33-h70-tanh-td-down's: not the same input twice)
    'rej-full-d16-h16-tanh-ti-down': 2,
    'h0-theta0-d10-h24-tanh-td-up': 7,
    'h0-d33-h70-tanh-td-up': 13,
    'grid-G1-d12-h14-tanh-ti-down': 2,
    'grid-G33-d40-h100-tanh-td-down': 2,
    'handle-0-d20-h40-tanh-ti-down': 2,
    'handle-0-d20-h40-tanh-td-down': 3,
    'handle-5-d20-h40-tanh-td': 2,
    'every-d17-h1-relu-td-up': 4,
}
TWEAKS = {
    'every-d17-h1-relu-td-up': dict(scale=1.5),          # (one hidden unit: at scale 1 the error ratios of both runs are roundoff)
    'tiny-B1-d3-h5-tanh-ti-down': dict(scale=4.0),       # (one row: at scale 3 the controller is steered by roundoff)
}

# a. every instantiation: batch 100 (four tiles, the last with 4 rows).  Per kernel three (dim, hidden): both ends of its range and one inside;
# each kernel sees every activation, both time-dependence settings and both time directions
_PER_DIM = ((('tanh', False, DOWN), ('relu', True, UP)),
            (('softplus', False, UP), ('tanh', True, DOWN)),
            (('relu', False, DOWN), ('softplus', True, DOWN), ('tanh', False, UP)))
EVERY = [_mk('every', dim, hd, 100, d, act=act, td=td) for box in BOXES.values() for i, (dim, hd) in enumerate(box) for act, td, d in _PER_DIM[i]]
TINY = [_mk('tiny-B%d' % b, dim, hd, b, DOWN) for dim, hd in ((3, 5), (64, 128)) for b in (1, 31)]

# b. natural grids, always with an 11-row last tile.  16 x 16: 128 threads, one thread group folds the partials, 8 at a time; 64 x 128: 512
# threads, four groups, 32 at a time.  (3, 5): 68 parameters - on a full grid most workgroups own no slice of theta
GRIDS_16, GRIDS_64 = (1, 2, 7, 8, 9, 17), (1, 4, 28, 29, 32, 33, 61)
GRIDS = ([_mk('grid-G%d' % n, 12, 14, ('G', n), DOWN) for n in GRIDS_16] +
         [_mk('grid-G%d' % n, 40, 100, ('G', n), DOWN, td=n in (4, 33)) for n in GRIDS_64] +
         [_mk('grid-GCUS-1', 3, 5, 'CUS-1', DOWN), _mk('grid-GCUS', 3, 5, 'CUS', DOWN), _mk('grid-GCUS', 20, 40, 'CUS', UP, td=True),
          _mk('grid-FULL', 16, 16, 'FULL', DOWN), _mk('grid-FULL', 64, 128, 'FULL', DOWN, td=True), _mk('grid-FULL3', 16, 16, 'FULL3', UP)])

# c. grids by override (MI_ODE_ADJOINT_GRID): batch 745 = 24 tiles, the last with 9 rows.  Grid 1: SL = P, hundreds of 128-element chunks of
# the slice fold; grid 5: 5, 5, 5, 5 and 4 tiles per workgroup
OVERRIDE_GRIDS = (1, 2, 5, 24)
OVERRIDE = [_mk('override', 10, 24, 745, DOWN), _mk('override', 48, 96, 745, UP, td=True)]

# d. rejected attempts: one case per kernel with a rejection AFTER an accepted step (the ping-pong slots s0_cur / th_cur and the FSAL planes of
# a later start state must stay put), one that rejects its first attempt, one whose interval ends inside the span of a rejected attempt (which
# wrote speculative dense output), one on a full grid
REJECTING = [_mk('rej', 16, 16, 100, DOWN, rejecting=True), _mk('rej', 8, 32, 100, DOWN, rejecting=True),
             _mk('rej', 64, 16, 100, DOWN, td=True, rejecting=True), _mk('rej', 33, 70, 100, DOWN, td=True, rejecting=True),
             _mk('rej-full', 16, 16, 'FULL', DOWN, rejecting=True)]
# relu: the initial step of misc.py:183-247 knows nothing of the kinks - the first attempts are rejected
REJECT_FIRST = _mk('rej-first', 33, 70, 100, DOWN, act='relu', rejecting=True)
# the interval of rej-d8-h32 cut at t0_r + 0.9 dt_r of its rejected attempt 9 (solver time is -t): the controller does not see t_end, so the
# attempts before it are the same, and attempt 9 - rejected - covers t_end
COVERED_T_END = Case('rej-covered-d8-h32-tanh-ti', 8, 32, 100, 1.0, 0.3406314911559536, seed=2, rejecting=True)
REJECTING += [REJECT_FIRST, COVERED_T_END]

# e. adj_t = 0 at the interval's start: the first guess h0 of the initial step is finite and the ADJ_INITB pass runs - with adj_params = 0
# (its scale is atol alone) and with 0.01 N(0, 1).  (A time-dependent network has a finite h0 in every case: adj_t has a derivative.)
FINITE_H0 = [_mk('h0', 10, 24, 200, DOWN, adjt=0.0, finite_h0=True), _mk('h0-theta0', 10, 24, 200, UP, td=True, adjt=0.0, th0=0.0, finite_h0=True),
             _mk('h0-theta0', 33, 70, 200, DOWN, adjt=0.0, th0=0.0, finite_h0=True), _mk('h0', 33, 70, 200, UP, td=True, adjt=0.0, finite_h0=True)]

# f. a long interval: 44 accepted steps of 54 attempts.  These networks are chaotic at the scales that keep the controller on truncation error:
# adj_y and adj_params grow by e^7 over the interval, and the float32 run's own deviation E32 with them.  a = 0.01 N(0, 1) / batch keeps
# max |adj_params| at 1e2; (scale 3, y = 2 N(0, 1), tolerance 1e-6, seed 8) is the admissible input with the most accepted steps of a search
# over scales 2 - 3, y scales 2 - 8, intervals 2 - 5 and eight seeds
LONG = _mk('long', 8, 32, 100, (0.0, 4.0), seed=8, scale=3.0, yscale=2.0, ascale=0.01, rtol=1e-6, atol=1e-6)


# g. one handle, these in order (same batch, widths, tolerances): tanh, relu, softplus, other weights, increasing time, decreasing time
def _handle(td):
    p = 'handle'
    return [_mk(p + '-0', 20, 40, 250, DOWN, td=td), _mk(p + '-1', 20, 40, 250, DOWN, act='relu', td=td),
            _mk(p + '-2', 20, 40, 250, DOWN, act='softplus', td=td), _mk(p + '-3-other-w', 20, 40, 250, DOWN, td=td, seed=4),
            _mk(p + '-4', 20, 40, 250, UP, td=td), _mk(p + '-5', 20, 40, 250, (0.9, 0.2), td=td)]


HANDLE, HANDLE_TD = _handle(False), _handle(True)

# h. status: a NaN in the ragged last tile, then the same engine on this clean case
STATUS = _mk('status', 20, 40, 100, DOWN)

SEGMENT_CASES = EVERY + TINY + GRIDS + OVERRIDE + REJECTING + FINITE_H0 + [LONG] + HANDLE + HANDLE_TD + [STATUS]
ALL_CASES = {c.name: c for c in SEGMENT_CASES}
assert len(ALL_CASES) == len(SEGMENT_CASES)


def ids(cases):
    return [c.name for c in cases]
