"""GPU tests of the tile boundary of the linear tile passes (csrc/mi_ode_step_fused.h: lin_attempt_pass, lin_f0_pass): the prefetched next
tile is consumed before the tile's stores, and the dense output reads its abscissae from a per-pass LDS table of kLinEmitCap entries
(lin_fill_emit / lin_emit) instead of forming them per element.  Neither changes a bit of any result, so every case asks for

  * the whole-call schedule (one launch) equal to options={'fusion': 'step'} bit for bit,
  * the numpy oracle's attempt and accept counts and max |got - ref| <= 1e-11 (float64) / 2e-4 (float32) - tests/test_gpu_linear_wide.py's bars,

on config 4's system (bench.py's matrix construction), rtol 1e-6, atol 1e-9, at the smallest shapes where the changed code can go wrong:
8197 rows at dim 128 (513 tiles on 256 workgroups: two to three tiles per workgroup, so the loop's back edge and the prefetch of the tile
after next both run, and the last tile is ragged by five rows), the same at dim 100 (lanes without a column), 33 rows at dim 16, float32 at
dim 128; with one output, about one and about eight outputs per attempt, more outputs in an attempt than the table holds (the in-place path),
exactly the table's capacity and one more, a rejected attempt whose speculative rows are overwritten, the non-plain path (bias, reversed
time), the tsit5 dense output (its table holds t itself) and bosh3, and odeint_adjoint on k_linadj (two attempt passes side by side)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import oracle.ode_numpy as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-6, atol=1e-9)
BAR = {'float64': 1e-11, 'float32': 2e-4}
SHAPES = [(8197, 128, 'float64'), (8197, 100, 'float64'), (33, 16, 'float64'), (8197, 128, 'float32')]
SHAPE_IDS = ['%dx%d-%s' % s for s in SHAPES]


def dev():
    return torch.device('cuda:0')


def emit_cap():
    """kLinEmitCap as the kernels were compiled with it."""
    src = open(os.path.join(ROOT, 'tfdiffeq_amd', 'csrc', 'mi_ode_step_fused.h')).read()
    return int(re.search(r'constexpr int kLinEmitCap = (\d+);', src).group(1))


@functools.lru_cache(maxsize=None)
def _system(batch, dim, dtype):
    """bench.py's config4() at another size: A = -I / 2 + (S - S^T) / (2 sqrt(dim)), f(t, y) = A y (+ b)."""
    S = torch.randn(dim, dim, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    A = -0.5 * torch.eye(dim, dtype=torch.float64) + 0.5 * (S - S.t()) / np.sqrt(dim)
    y0 = torch.randn(batch, dim, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    b = 0.1 * torch.randn(dim, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    dt = getattr(torch, dtype)
    return A.to(dt), y0.to(dt), b.to(dt)


@functools.lru_cache(maxsize=None)
def _oracle(batch, dim, dtype, tt, method, bias, first_step):
    """(solution, statistics) of the numpy oracle; computed once per case and shared (the result is never modified)."""
    A, y0, b = _system(batch, dim, dtype)
    An, bn = A.numpy(), b.numpy()
    fo = (lambda t_, y: y @ An.T + bn) if bias else (lambda t_, y: y @ An.T)
    opts = {}
    if method == 'tsit5':
        opts['tsit5_fixed'] = True                             # (the product integrates with the published tsit5 tableau)
    if first_step is not None:
        opts['first_step'] = first_step
    ref, st = O.odeint(fo, y0.numpy(), np.array(tt).astype(An.dtype), method=method, return_stats=True, options=opts or None, **TOL)
    ref.setflags(write=False)
    return ref, st


def _check(batch, dim, dtype, tt, method='dopri5', bias=False, first_step=None, counts=None, same_counts=True):
    """Both schedules on the GPU against each other (bits) and against the oracle; returns the oracle's statistics."""
    from tfdiffeq_amd import odeint, rhs
    A, y0, b = _system(batch, dim, dtype)
    ref, st_ref = _oracle(batch, dim, dtype, tuple(float(v) for v in tt), method, bias, first_step)
    f = rhs.Linear.from_matrix(A, b if bias else None)
    t = torch.tensor(np.array(tt, dtype=np.float64))
    sols = {}
    for fusion in ('auto', 'step'):
        opts = {'fusion': fusion}
        if first_step is not None:
            opts['first_step'] = first_step
        sol = odeint(f, y0.to(dev()), t, method=method, options=opts, **TOL)
        st = dict(odeint.last_stats)
        sols[fusion] = sol.cpu()
        diff = float(np.abs(sols[fusion].numpy() - ref).max())
        print('%d x %d %s %s, %d outputs, %s: attempts %d accepted %d launches %d (oracle %d / %d), max |got - ref| %.3e (bar %.0e)'
              % (batch, dim, dtype, method, len(tt), fusion, st['n_attempts'], st['n_accepted'], st['n_launches'], st_ref.n_attempts,
                 st_ref.n_accepted, diff, BAR[dtype]))
        if fusion == 'auto':
            assert st['n_launches'] == 1, st
        if same_counts:
            assert (st['n_attempts'], st['n_accepted']) == (st_ref.n_attempts, st_ref.n_accepted), (fusion, st, vars(st_ref))
        assert diff <= BAR[dtype], (fusion, diff)
    assert torch.equal(sols['auto'], sols['step']), float((sols['auto'] - sols['step']).abs().max())
    if counts is not None:
        assert (st_ref.n_attempts, st_ref.n_accepted) == counts, vars(st_ref)
    return st_ref


GRIDS = [[0., 1.], list(np.linspace(0., 1., 5)), list(np.linspace(0., 1., 41))]


@pytest.mark.parametrize('tt', GRIDS, ids=['T2', 'T5', 'T41'])
@pytest.mark.parametrize('batch,dim,dtype', SHAPES, ids=SHAPE_IDS)
def test_one_to_eight_outputs_per_attempt(batch, dim, dtype, tt):
    """One output in the last attempt only; five attempts with about one and about eight outputs each (the table path)."""
    st = _check(batch, dim, dtype, tt)
    if dtype == 'float64' and dim >= 100:
        assert st.n_attempts == 5, vars(st)


@pytest.mark.parametrize('dim', [16, 128])
def test_more_outputs_in_an_attempt_than_the_table_holds(dim):
    """1501 output times over five or so attempts: every attempt has far more outputs than the table holds and forms its abscissae in place.
    (33 rows: the solution has 1501 of them.)"""
    assert 1500 // 8 > emit_cap()
    _check(33, dim, 'float64', list(np.linspace(0., 1., 1501)))


@pytest.mark.parametrize('extra', [0, 1], ids=['capacity', 'capacity+1'])
@pytest.mark.parametrize('batch,dim,dtype', [SHAPES[0], SHAPES[2], SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[2], SHAPE_IDS[3]])
def test_exactly_the_capacity_of_the_table_and_one_more(batch, dim, dtype, extra):
    """The first attempt is `first_step` = 0.05 long and accepted (no attempt of the call is rejected); n = capacity (+ 1) output times lie
    strictly inside it, the next one is t = 1: the first attempt emits exactly n outputs - the last size on the table, the first beyond."""
    n = emit_cap() + extra
    h = 0.05
    tt = [0.] + [h * (i + 0.5) / n for i in range(n)] + [1.]
    st = _check(batch, dim, dtype, tt, first_step=h)
    assert st.n_attempts == st.n_accepted, vars(st)


@pytest.mark.parametrize('batch,dim,counts', [(8197, 128, (5, 4)), (8197, 100, (5, 4)), (33, 16, (4, 3))], ids=SHAPE_IDS[:3])
def test_rejected_first_attempt_is_overwritten(batch, dim, counts):
    """first_step = 0.9 is rejected: the attempt wrote nothing final - no output falls into it here, and y1 / f1 are written again."""
    _check(batch, dim, 'float64', [0., 1.], first_step=0.9, counts=counts)


@pytest.mark.parametrize('batch,dim', [(8197, 128), (33, 16)], ids=[SHAPE_IDS[0], SHAPE_IDS[2]])
def test_rejected_attempt_with_speculative_outputs(batch, dim):
    """... and with outputs inside the rejected attempt: its speculative rows are overwritten by the accepted steps that cover them."""
    st = _check(batch, dim, 'float64', list(np.linspace(0., 1., 5)), first_step=0.9)
    assert st.n_attempts > st.n_accepted, vars(st)


@pytest.mark.parametrize('tt', [[1., 0.], list(np.linspace(1., 0., 5))], ids=['T2', 'T5'])
@pytest.mark.parametrize('batch,dim,dtype', [SHAPES[0], SHAPES[2], SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[2], SHAPE_IDS[3]])
def test_bias_and_reversed_time(batch, dim, dtype, tt):
    """The non-plain evaluation (bias add, sign product) under the same tile loop."""
    _check(batch, dim, dtype, tt, bias=True)


@pytest.mark.parametrize('batch,dim,dtype', [SHAPES[0], SHAPES[2]], ids=[SHAPE_IDS[0], SHAPE_IDS[2]])
def test_tsit5_dense_output(batch, dim, dtype):
    """tsit5's seven-weight dense output: the table holds t itself."""
    _check(batch, dim, dtype, list(np.linspace(0., 1., 5)), method='tsit5')


def test_tsit5_dense_output_float32_states():
    """... with float32 states the table still holds t in float64 (tsit5_dense forms its weights in float64): an instantiation of its own.
    The oracle is no float32 reference for this tableau - its coefficient arrays promote a float32 state to float64 in the first stage
    (the result it returns is float64, asserted here so that the exemption ends with its reason), and its step sequence is that of
    neither precision (14 attempts / 8 accepted; 12 / 7 in float64, which is also what the kernels take in float32: 12 / 7 measured on
    the MI355X).  So this case asks for everything but the counts: one launch, both schedules bit for bit, the float32 bar."""
    batch, dim, dtype = SHAPES[3]
    tt = list(np.linspace(0., 1., 5))
    ref, _ = _oracle(batch, dim, dtype, tuple(float(v) for v in tt), 'tsit5', False, None)
    assert ref.dtype == np.float64
    _check(batch, dim, dtype, tt, method='tsit5', same_counts=False)


@pytest.mark.parametrize('batch,dim,dtype', [(8197, 16, 'float64'), (33, 16, 'float64'), (8197, 16, 'float32')])
def test_bosh3_three_stages(batch, dim, dtype):
    """bosh3 takes 400 and more steps over [0, 1] at these tolerances, so the oracle decides the shape: dim 16, where 8197 rows still give
    every workgroup two to three tiles and the oracle less than a second of work (at dim 128 it needs 48 s)."""
    _check(batch, dim, dtype, list(np.linspace(0., 1., 5)), method='bosh3')


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def test_linear_adjoint_one_launch_against_the_callable_engine():
    """odeint_adjoint of y @ W at 8197 x 128: k_linadj runs two attempt passes side by side, one per half of its grid, and its f0 pass also
    prefetches the output gradient.  Against the callable engine (adjoint.LINEAR_ONE_LAUNCH = False) at tests/test_gpu_linadj_edges.py's 1e-11."""
    from tfdiffeq_amd import adjoint as ADJ
    from tfdiffeq_amd import models, odeint_adjoint
    ADJ.clear_adjoint_engines()
    try:
        torch.manual_seed(128)
        func = models.LinearODEFunc(128, bias=False, dtype=torch.float64).to(dev())
        g = torch.Generator().manual_seed(8197)
        y0 = torch.randn(8197, 128, generator=g, dtype=torch.float64).to(dev())
        t = torch.tensor([0., 0.6, 1.], dtype=torch.float64)
        w = torch.randn(3, 8197, 128, generator=g, dtype=torch.float64).to(dev())
        res = []
        for one_launch in (True, False):
            ADJ.LINEAR_ONE_LAUNCH = one_launch
            for p in func.parameters():
                p.grad = None
            yi = y0.clone().requires_grad_(True)
            tt = t.clone().requires_grad_(True)
            sol = odeint_adjoint(func, yi, tt, rtol=1e-7, atol=1e-9, method='dopri5')
            (sol * w).sum().backward()
            res.append((yi.grad.clone(), [p.grad.clone() for p in func.parameters()], tt.grad.clone(), dict(odeint_adjoint.last_backward_stats)))
        a, b = res
        assert a[3]['engine'].startswith('linear right-hand side: one launch per interval'), a[3]['engine']
        assert b[3]['engine'].startswith('linear right-hand side: augmented dynamics on the MFMA kernels'), b[3]['engine']
        assert all(s_['n_launches'] == 1 and s_['status'] == 0 for s_ in a[3]['segments'])
        assert a[3]['segments'][-1]['n_attempts'] == b[3]['last_segment']['n_attempts']
        figs = [_rel(a[0], b[0])] + [_rel(x, y) for x, y in zip(a[1], b[1])] + [float((a[2] - b[2]).abs().max()) / max(1.0, float(b[2].abs().max()))]
        print('k_linadj at 8197 x 128 against the callable engine: dL/dy0 %.3e, parameters %s, dL/dt %.3e (bar 1e-11)'
              % (figs[0], ' '.join('%.3e' % v for v in figs[1:-1]), figs[-1]))
        assert max(figs) < 1e-11, figs
    finally:
        ADJ.LINEAR_ONE_LAUNCH = True
        ADJ.clear_adjoint_engines()
