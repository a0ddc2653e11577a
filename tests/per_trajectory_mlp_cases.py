"""Inputs of the per-trajectory MLP tests (tests/test_gpu_per_trajectory_mlp.py; csrc/mi_ode_rows_mlp.h, k_rows_mlp): seeded ODEFunc-shaped
networks on every tile geometry, batches around the 32-row tile, rows made heterogeneous by scaling y0 over two decades so that the rows'
own attempt counts differ (checked on the CPU with the float64 oracle: `python tests/per_trajectory_mlp_cases.py` prints them).

Everything here is host-side: numpy weights, a numpy right-hand side for the oracle (oracle/rhs_numpy.py's `mlp_tanh` where the case is a
time-independent tanh net, the same three lines with the case's activation and time input elsewhere)."""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOL = dict(rtol=1e-4, atol=1e-6)                              # the float32 tests' tolerances (tests/test_gpu_per_trajectory.py)
# the oracle cases.  bands.case_ceiling allows 8 x eps32 x (S + 1) = 3.3e-6 (dopri5, tsit5; bosh3: 1.9e-6) per attempt for ROUNDING.  An adaptive solve also has
# its own error: up to its tolerance per accepted step, so two solves of one row whose step sequences fork on one rounding (the float32
# kernel and the float64 oracle do) differ by up to attempts x (rtol |y| + atol) - with TOL that is 30 x the ceiling, whatever the kernel
# does.  The tolerance of these cases therefore keeps the solver's own error per attempt under a third (bosh3: about half) of the rounding allowance:
# rtol 1e-6, atol 1e-8 (float32 still resolves it: the error estimate's own rounding is about a tenth of that).  (History: at rtol 1e-5 /
# atol 1e-7 - argued from a fork costing ONE tolerance, not one per step - two of 27 sampled rows missed, both rows whose step sequence
# forked or nearly did: cragged_softplus_b33_tsit5_tdep row 17, 16 attempts against the oracle's 15, 1.04e-4 against 5.0e-5, and
# cfull_tanh_b70_dopri5_tdep_grid2 row 17, 6.6e-5 against 5.7e-5; every row was bit-equal to the shared kernel's batch-of-one call.)
TOL_ORACLE = dict(rtol=1e-6, atol=1e-8)
STAGES = {'dopri5': 6, 'tsit5': 6, 'bosh3': 3}                # S: the a-priori ceiling takes stages = S + 1
GAIN = 1.5                                                    # weight scale: enough curvature for a dozen or more attempts per row

Case = collections.namedtuple('Case', 'name dim hidden act tdep batch method t opts contractive', defaults=(False,))

# horizons per tableau, so that a row needs between a handful and ~150 attempts: dopri5 and tsit5 [0, 3]; bosh3 [0, 1]
T2 = [0., 3.]
T5 = [0., 0.75, 1.5, 2.25, 3.0]
T5_REV = T5[::-1]
T5_B = [0., 0.25, 0.5, 0.75, 1.0]
T5_B_REV = T5_B[::-1]
T40 = [float(v) for v in np.linspace(0., 2.0, 40)]            # closely spaced: a row emits several outputs inside one accepted step


def _c(name, dim, hidden, act, tdep, batch, method, t, **opts):
    return Case(name, dim, hidden, act, tdep, batch, method, t, opts)


# (dim, hidden) on every instantiated geometry: (3, 5) -> 16 x 16, (20, 100) -> 64 x 128 ragged, (64, 128) full, (64, 16), (16, 128);
# batches 1, 31, 32, 33, 70; the three tableaus; the three activations (on 16 x 16 and on 64 x 128); with and without the time input;
# forward and reversed t; T = 1, 2, 5, 40; the grid clamped to 1 and 2 workgroups at batch 70 (3 tiles)
CASES = [
    _c('g16x16_tanh_b70_dopri5', 3, 5, 'tanh', False, 70, 'dopri5', T5),
    _c('g16x16_relu_b33_tsit5_tdep', 3, 5, 'relu', True, 33, 'tsit5', T5),
    _c('g16x16_softplus_b31_bosh3', 3, 5, 'softplus', False, 31, 'bosh3', [0., 1.]),
    _c('ragged_tanh_b70_dopri5_tdep_grid1', 20, 100, 'tanh', True, 70, 'dopri5', T5, rows_grid=1),
    _c('ragged_relu_b32_bosh3_rev', 20, 100, 'relu', False, 32, 'bosh3', T5_B_REV),
    _c('full_tanh_b70_tsit5_grid2', 64, 128, 'tanh', False, 70, 'tsit5', T5, rows_grid=2),
    _c('full_softplus_b33_dopri5_tdep_rev', 64, 128, 'softplus', True, 33, 'dopri5', T5_REV),
    _c('full_relu_b1_dopri5', 64, 128, 'relu', False, 1, 'dopri5', T2),
    _c('g64x16_tanh_b33_dopri5_T40', 64, 16, 'tanh', False, 33, 'dopri5', T40),
    _c('g64x16_tanh_b31_tsit5_T40_tdep', 64, 16, 'tanh', True, 31, 'tsit5', T40),
    _c('g16x128_tanh_b32_bosh3_tdep', 16, 128, 'tanh', True, 32, 'bosh3', T5_B),
    _c('g16x128_tanh_b70_dopri5_T1', 16, 128, 'tanh', False, 70, 'dopri5', [0.5]),
]
# the cases held to the batch-of-one call on the shared kernel: every geometry, every tableau, every activation, both time modes, both directions
SHARED_CASES = ['g16x16_tanh_b70_dopri5', 'ragged_tanh_b70_dopri5_tdep_grid1', 'full_tanh_b70_tsit5_grid2', 'g64x16_tanh_b33_dopri5_T40',
                'g16x128_tanh_b32_bosh3_tdep', 'ragged_relu_b32_bosh3_rev', 'full_softplus_b33_dopri5_tdep_rev']
# ... and to the float64 oracle.  The a-priori ceiling bands.case_ceiling(attempts, stages) takes growth = 1: rounding errors are not amplified
# by the dynamics.  The dense random nets above amplify a perturbation 14 - 60 times over their horizon (measured with the oracle), so the
# oracle cases are nets that PROVABLY do not: W2 = diag(u), u > 0, W3 = -W1_y^T (W1 without its time row) give the Jacobian
# -W1_y D1 U D2 W1_y^T with D1, D2 >= 0 the activations' derivatives - symmetric negative semi-definite for every t and y, so the distance
# between two solutions never grows.  One per geometry, every tableau, every activation, both time modes.  (method='tsit5' is the published
# tableau: the oracle's options['tsit5_fixed'], as in tests/test_gpu_parity.py.)
ORACLE = [
    _c('c16x16_tanh_b70_dopri5', 3, 5, 'tanh', False, 70, 'dopri5', T5),
    _c('cragged_softplus_b33_tsit5_tdep', 20, 100, 'softplus', True, 33, 'tsit5', T5),
    _c('cfull_tanh_b70_dopri5_tdep_grid2', 64, 128, 'tanh', True, 70, 'dopri5', T5, rows_grid=2),
    _c('c64x16_relu_b33_bosh3', 64, 16, 'relu', False, 33, 'bosh3', T5_B),
    _c('c16x128_tanh_b32_dopri5_T40', 16, 128, 'tanh', False, 32, 'dopri5', T40),
]
ORACLE = [c._replace(contractive=True) for c in ORACLE]
ORACLE_CASES = [c.name for c in ORACLE]
BY_NAME = {c.name: c for c in CASES + ORACLE}


def tol(case):
    return TOL_ORACLE if case.contractive else TOL


def _seed(case):
    return int(sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) % (2 ** 31))


def weights(case):
    """W1 [dim (+ 1), hidden], b1, W2, b2, W3, b3 as float32 numpy arrays ([in, out], Keras Dense layout; row 0 of W1 multiplies t)."""
    rng = np.random.default_rng(_seed(case))
    d, h = case.dim, case.hidden
    W1 = rng.standard_normal((d + (1 if case.tdep else 0), h)) * (GAIN / np.sqrt(d))
    W2 = rng.standard_normal((h, h)) * (GAIN / np.sqrt(h))
    W3 = rng.standard_normal((h, d)) * (GAIN / np.sqrt(h))
    if case.contractive:                                      # a gradient-like flow: see ORACLE
        W2 = np.diag(rng.uniform(0.5, 1.5, h))
        W3 = -W1[-d:].T
    b1, b2, b3 = 0.1 * rng.standard_normal(h), 0.1 * rng.standard_normal(h), 0.1 * rng.standard_normal(d)
    return [a.astype(np.float32) for a in (W1, b1, W2, b2, W3, b3)]


def scales(batch):
    """Row scales over two decades, 0.1 .. 10, in a fixed shuffled order (neighbours in a tile differ)."""
    s = np.logspace(-1.0, 1.0, batch) if batch > 1 else np.array([1.0])
    return s[np.random.default_rng(7).permutation(batch)]


def y0(case):
    rng = np.random.default_rng(_seed(case) + 1)
    return (rng.standard_normal((case.batch, case.dim)) * scales(case.batch)[:, None]).astype(np.float32)


def perm(batch):
    return np.random.default_rng(11).permutation(batch)


def sample_rows(batch):
    """A fixed sample: the tile edges (0, 31, 32, last) and two rows inside."""
    return sorted({i for i in (0, 5, 17, 31, 32, 33, batch - 1) if 0 <= i < batch})


_ACT = {'tanh': np.tanh, 'relu': lambda z: np.maximum(z, 0.0), 'softplus': lambda z: np.logaddexp(z, 0.0)}


def numpy_rhs(case, dtype=np.float64):
    """The case's network for the oracle, in `dtype`."""
    W1, b1, W2, b2, W3, b3 = [np.asarray(a, dtype=dtype) for a in weights(case)]
    if case.act == 'tanh' and not case.tdep:
        from oracle.rhs_numpy import make_rhs
        return make_rhs('mlp_tanh', dtype=dtype, weights=dict(W1=W1, b1=b1, W2=W2, b2=b2, W3=W3, b3=b3))
    act = _ACT[case.act]

    def mlp(t, y):
        x = y
        if case.tdep:                                         # dense_odenet.py:79-84: fc1 sees concat([t, x])
            x = np.concatenate([np.ones(y.shape[:-1] + (1,), dtype=y.dtype) * np.asarray(t, dtype=y.dtype), y], axis=-1)
        h = act(x @ W1 + b1)
        h = act(h @ W2 + b2)
        return h @ W3 + b3
    return mlp


_ORACLE = {}


def oracle_rows(case, rows=None):
    """The float64 oracle on every sampled row ALONE: ({row: solution [T, dim]}, {row: (attempts, accepted)}), computed once per case."""
    from oracle import ode_numpy as O
    key = (case.name, tuple(rows) if rows is not None else None)
    if key not in _ORACLE:
        f, y, sols, counts = numpy_rhs(case), y0(case).astype(np.float64), {}, {}
        for i in (rows if rows is not None else range(case.batch)):
            ref, st = O.odeint(f, y[i:i + 1], np.asarray(case.t), method=case.method, return_stats=True,
                               options={'tsit5_fixed': True} if case.method == 'tsit5' else None, **tol(case))
            sols[i], counts[i] = ref[:, 0], (st.n_attempts, st.n_accepted)
        _ORACLE[key] = (sols, counts)
    return _ORACLE[key]


if __name__ == '__main__':
    for c_ in CASES + ORACLE:
        if len(c_.t) < 2:
            continue
        _, cnt = oracle_rows(c_, sample_rows(c_.batch))
        print('%-40s attempts per sampled row %s' % (c_.name, [cnt[i][0] for i in sorted(cnt)]))
