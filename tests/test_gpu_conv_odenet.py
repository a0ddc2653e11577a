"""The fused convolutional stage kernel (csrc/mi_ode_conv.h, rhs.Conv2dODE) and the conv models on the MI355X: against the torch
module and the float64 numpy restatement (tests/conv_restatement.py), through every solver family, under hipGraph replay and in
training."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_restatement as CR  # noqa: E402
from tfdiffeq_amd import models, odeint, odeint_adjoint  # noqa: E402
from tfdiffeq_amd.misc import _lincomb  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32_BAND = 2e-5          # float32: |got - ref| <= band * (1 + |ref|) against the float64 restatement (three convs of <= 9 x 128 terms)


def _func(C_, F, aug=0, td=False, act='relu', dtype=torch.float64, seed=0):
    torch.manual_seed(seed)
    fn = models.Conv2dODEFunc(C_, F, augment_dim=aug, time_dependent=td, non_linearity=act)
    with torch.no_grad():
        for p in fn.parameters():
            p.mul_(2.0)
    return fn.to(DEV, dtype)


def _y(B, C_, H, W, dtype=torch.float64, seed=1):
    return torch.randn(B, C_, H, W, dtype=dtype, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _rel(a, b):
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


CASES = [(10, 3, 5, 5, 10), (4, 1, 28, 28, 92), (2, 6, 28, 28, 64), (2, 3, 32, 32, 125), (2, 13, 32, 32, 64), (3, 13, 7, 5, 92),
         (2, 2, 1, 1, 16)]


@pytest.mark.parametrize('act', ['relu', 'softplus', 'tanh'])
@pytest.mark.parametrize('td', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_fused_evaluation_matches_module_and_restatement(act, td, case):
    B, C_, H, W, F = case
    for dtype in (torch.float64, torch.float32):
        fn = _func(C_, F, td=td, act=act, dtype=dtype)
        desc = fn.device_rhs()
        y = _y(B, C_, H, W, dtype)
        for t in (0.7, -1.3):
            tt = torch.tensor(t, dtype=dtype, device=DEV)
            with torch.no_grad():
                got = desc(tt, y)
                mod = fn(tt, y)
            ref = torch.from_numpy(CR.f(CR.params(fn), t, y.double().cpu().numpy(), act, td)).to(DEV)
            if dtype == torch.float64:
                assert _rel(got, mod) <= 1e-12 and _rel(got, ref) <= 1e-12, (case, t)
            else:
                assert float(((got.double() - ref).abs() / (1 + ref.abs())).max()) <= F32_BAND, (case, t)
            rev = desc.reversed()                                      # a reversed axis: -f(-t, y)
            with torch.no_grad():
                assert torch.equal(rev(-tt, y), -got)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_stage_state_is_bit_identical_to_lincomb(dtype):
    fn = _func(5, 32, td=True, act='tanh', dtype=dtype)
    desc = fn.device_rhs()
    y0 = _y(3, 5, 11, 9, dtype)
    ks = [_y(3, 5, 11, 9, dtype, seed=s) for s in range(2, 8)]
    beta = [0.1, -0.3, 0.25, 1.7, -0.9, 0.05]
    dt = torch.tensor(0.137, dtype=torch.float64, device=DEV)
    t = torch.tensor(0.4, dtype=dtype, device=DEV)
    k, ys = desc.stage(t, y0, ks, beta, dt, want_y=True)
    ref = _lincomb(y0, beta, ks, dt)
    assert torch.equal(ys, ref)
    with torch.no_grad():
        assert torch.equal(k, desc(t, ref))


@pytest.mark.parametrize('method', ['dopri5', 'tsit5', 'bosh3', 'adaptive_heun', 'dopri8'])
def test_adaptive_solves_match_module_on_callable_engine(method):
    fn = _func(3, 16, td=True, act='softplus')
    y0 = _y(4, 3, 9, 7) * 0.5
    t = torch.tensor([0., 0.5, 1.0], dtype=torch.float64)
    kw = dict(rtol=1e-7, atol=1e-9, method=method)
    with torch.no_grad():
        ref = odeint(fn, y0, t, options={'graph': False}, **kw)
        s_ref = dict(odeint.last_stats)
        got = odeint(fn.device_rhs(), y0, t, options={'graph': False}, **kw)
        s_got = dict(odeint.last_stats)
    # the descriptor took the one-launch stage path (graph_step.DeviceControlledRK.stage_rhs): no Python evaluation per stage
    assert 'fused stage kernel' in s_got['engine'] and s_got['python_evaluations'] == 0, s_got
    assert 'one Python evaluation per stage' in s_ref['engine'] and s_ref['python_evaluations'] > 0, s_ref
    counts = [(s.get('n_accepted'), s.get('n_rejected'), s.get('n_attempts')) for s in (s_got, s_ref)]
    assert counts[0] == counts[1] and counts[0][0], (s_got, s_ref)
    assert _rel(got, ref) <= 1e-10


@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4', 'fixed_adams'])
def test_fixed_grid_and_adams_match_module(method):
    fn = _func(2, 24, act='tanh')
    y0 = _y(3, 2, 6, 6) * 0.5
    for t in (torch.linspace(0., 1., 6, dtype=torch.float64), torch.tensor([1., 0.], dtype=torch.float64)):
        with torch.no_grad():
            ref = odeint(fn, y0, t, method=method, options={'step_size': 0.05})
            got = odeint(fn.device_rhs(), y0, t, method=method, options={'step_size': 0.05})
        assert _rel(got, ref) <= 1e-12, (method, t)


@pytest.mark.parametrize('F', [32, 128])          # (float64, F = 128: 116 KB of LDS - the raised dynamic-LDS limit, under capture too)
def test_graph_replay_is_bit_identical_to_eager(F):
    fn = _func(3, F, td=True, act='relu')
    desc = fn.device_rhs()
    y0 = _y(2, 3, 12, 12) * 0.5
    t = torch.tensor([0., 1., 2.], dtype=torch.float64)
    with torch.no_grad():
        eager = odeint(desc, y0, t, rtol=1e-8, atol=1e-10, method='dopri5', options={'graph': False})
        assert 'fused stage kernel' in odeint.last_stats['engine'] and odeint.last_stats['python_evaluations'] == 0
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            rec = odeint(desc, y0, t, rtol=1e-8, atol=1e-10, method='dopri5', options={'graph': True})
    assert 'hipGraph' in odeint.last_stats['engine'] and odeint.last_stats['python_evaluations'] == 0, odeint.last_stats
    assert torch.equal(eager, rec)
    with torch.no_grad():                                             # a reversed axis through the wrapper's reversed descriptor
        back = odeint(desc, rec[-1], torch.tensor([2., 0.], dtype=torch.float64), rtol=1e-8, atol=1e-10, method='dopri5', options={'graph': False})
        assert 'fused stage kernel' in odeint.last_stats['engine'] and odeint.last_stats['python_evaluations'] == 0   # (_ReverseFunc.stage_rhs)
        back_ref = odeint(fn, rec[-1], torch.tensor([2., 0.], dtype=torch.float64), rtol=1e-8, atol=1e-10, method='dopri5', options={'graph': False})
    assert _rel(back, back_ref) <= 1e-8            # (rtol: relu's kinks carry the kernel's last-bit differences from torch's convs)


@pytest.mark.parametrize('td', [False, True])
def test_reference_model_cases(td):
    torch.manual_seed(0)
    model = models.Conv2dODENet((3, 5, 5), num_filters=10, output_dim=2, time_dependent=td).to(DEV)
    x = torch.zeros(10, 3, 5, 5, device=DEV)
    with torch.no_grad():
        y = model(x)
    assert tuple(y.shape) == (10, 2, 5, 5)
    assert model.odeblock.odefunc.nfe > 0
    assert 'fused stage kernel' in odeint.last_stats['engine'] and odeint.last_stats['python_evaluations'] == 0   # ODEBlock's route
    aug = models.Conv2dODENet((3, 5, 5), num_filters=10, output_dim=2, augment_dim=2, time_dependent=td).to(DEV)
    with torch.no_grad():
        feats, pred = aug(torch.randn(4, 3, 5, 5, device=DEV), return_features=True)
        traj = aug.odeblock.trajectory(torch.randn(4, 3, 5, 5, device=DEV), 7)
    assert tuple(feats.shape) == (4, 5, 5, 5) and tuple(pred.shape) == (4, 2, 5, 5) and tuple(traj.shape) == (7, 4, 5, 5, 5)
    x = torch.randn(6, 3, 5, 5, device=DEV)
    with torch.no_grad():
        fused = aug.odeblock(x)
        with torch.no_grad():
            ref = odeint(aug.odeblock.odefunc, torch.cat([x, torch.zeros(6, 2, 5, 5, device=DEV)], 1),
                         torch.tensor([0., 1.]), rtol=1e-3, atol=1e-3, method='dopri5', options={'max_num_steps': 1000})[1]
    assert float(((fused - ref).abs() / (1 + ref.abs())).max()) <= 1e-4


def _rk4_loop(fn, y, n=16):
    h = 1.0 / n
    t = 0.0
    for _ in range(n):                                                 # rk_common.rk4_alt_step_func (the 3/8 rule)
        k1 = fn(torch.tensor(t, dtype=y.dtype, device=y.device), y)
        k2 = fn(torch.tensor(t + h / 3, dtype=y.dtype, device=y.device), y + h * k1 / 3)
        k3 = fn(torch.tensor(t + 2 * h / 3, dtype=y.dtype, device=y.device), y + h * (k2 - k1 / 3))
        k4 = fn(torch.tensor(t + h, dtype=y.dtype, device=y.device), y + h * (k1 - k2 + k3))
        y = y + h * (k1 + 3 * (k2 + k3) + k4) / 8
        t += h
    return y


@pytest.mark.parametrize('adjoint', [True, False])
def test_training_gradients_match_autograd_through_rk4(adjoint):
    fn = _func(2, 8, aug=1, td=True, act='tanh')
    block = models.ODEBlock(fn, is_conv=True, adjoint=adjoint, solver='rk4')
    block.options = {'step_size': 1.0 / 16}
    x = _y(2, 2, 5, 4).requires_grad_(True)
    block(x).pow(2).sum().backward()
    got = [p.grad.clone() for p in fn.parameters()] + [x.grad.clone()]
    for p in fn.parameters():
        p.grad = None
    x2 = x.detach().clone().requires_grad_(True)
    _rk4_loop(fn, torch.cat([x2, torch.zeros(2, 1, 5, 4, dtype=x2.dtype, device=DEV)], 1)).pow(2).sum().backward()
    ref = [p.grad for p in fn.parameters()] + [x2.grad]
    for g, r in zip(got, ref):
        assert _rel(g, r) <= 1e-5      # the continuous adjoint (a backward RK4 solve) against autograd through the forward loop: O(h^4), h = 1/16


def test_outside_box_runs_torch_and_warns_once():
    from tfdiffeq_amd import rhs
    rhs.Conv2dODE._told_limits.clear()
    for F, act in ((160, 'relu'), (16, 'elu')):
        fn = _func(2, F, act=act)
        block = models.ODEBlock(fn, is_conv=True, tol=1e-6)
        x = _y(2, 2, 6, 6)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            with torch.no_grad():
                got = block(x)
                block(x)
        assert sum('Conv2dODE' in str(m.message) for m in w) == 1
        with torch.no_grad():
            ref = odeint(fn, x, torch.tensor([0., 1.], dtype=torch.float64), rtol=1e-6, atol=1e-6, method='dopri5', options={'max_num_steps': 1000})[1]
        assert torch.equal(got, ref)


def test_odeblock_routes_large_shapes_to_torch():
    """Above rhs.Conv2dODE.FUSED_MAX_CONV2_FLOP of conv2 per evaluation the fused kernel measured slower: ODEBlock runs the module."""
    fn = _func(1, 64, act='relu', dtype=torch.float32)
    desc = fn.device_rhs()
    per_image = desc.conv2_flop(torch.empty(1, 1, 28, 28))
    for B, fused in ((max(1, int(desc.FUSED_MAX_CONV2_FLOP // per_image)), True), (int(desc.FUSED_MAX_CONV2_FLOP // per_image) + 1, False)):
        block = models.ODEBlock(fn, is_conv=True)
        with torch.no_grad():
            block(_y(B, 1, 28, 28, torch.float32))
        assert ('fused stage kernel' in str(odeint.last_stats.get('engine'))) == fused, (B, odeint.last_stats.get('engine'))
