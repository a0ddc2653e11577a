"""GPU tests of the hypersolvers: the fused one-launch engine (csrc/mi_ode_hyper.h) against a float64 numpy restatement of the
reference's euler.py (tests/hyper_restatement.py), against odeint's Euler, and against the eager (autograd) engine."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import hyper_restatement as HR
from tfdiffeq_amd import hyper_solvers as H
from tfdiffeq_amd import odeint, plugin_examples, rhs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SOLVERS = {'euler': H.HyperEuler, 'midpoint': H.HyperMidpoint, 'heun': H.HyperHeun}
F32_BAND = 2e-4          # float32 kernels against the float64 restatement (129 steps; measured well inside)


def make_g(kind, d, dtype=torch.float64, seed=0):
    torch.manual_seed(seed)
    n = 2 * d + 1
    if kind == 'notebook':
        g = nn.Sequential(nn.Linear(n, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, d))
        with torch.no_grad():
            for m in g:
                if isinstance(m, nn.PReLU):
                    m.weight.uniform_(0.05, 0.5)           # per channel, distinct
    elif kind == 'tanh50':
        g = nn.Sequential(nn.Linear(n, 50), nn.Tanh(), nn.Linear(50, d))
    else:
        g = nn.Sequential(nn.Linear(n, 128), nn.Softplus(), nn.Linear(128, 128), nn.Softplus(), nn.Linear(128, d))
    return g.to(device=DEV, dtype=dtype).requires_grad_(False)


F_CASES = {
    'lorenz': (lambda: rhs.Lorenz(), 3, HR.lorenz, {}),
    'vdp_plugin': (lambda: plugin_examples.van_der_pol(5.0), 2, HR.van_der_pol, {}),
    'lorenz_callable': (lambda: HR.lorenz_torch, 3, HR.lorenz, {'lower': True}),
}


def y0_for(d, B, seed=1):
    rng = np.random.default_rng(seed)
    base = np.array([1., 1., 1.]) if d == 3 else np.array([2., 0.])
    return base + 0.1 * rng.standard_normal((B, d))


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


T129 = np.linspace(0., 1., 129)


@pytest.mark.parametrize('B', [1, 37, 4096])
@pytest.mark.parametrize('gk', ['notebook', 'tanh50', 'softplus128'])
@pytest.mark.parametrize('fk', list(F_CASES))
@pytest.mark.parametrize('method', list(SOLVERS))
def test_fused_trajectory_matches_the_restatement(method, fk, gk, B):
    mk, d, fnp, opts = F_CASES[fk]
    g = make_g(gk, d)
    s = SOLVERS[method](mk(), g, options=opts)
    y0 = y0_for(d, B)
    out = s.trajectory(torch.tensor(T129, device=DEV), torch.tensor(y0, device=DEV))
    assert s.last_stats['engine'] == 'fused', s.last_stats
    assert tuple(out.shape) == (129, B, d)
    ref = HR.trajectory(method, fnp, HR.g_layers(g), T129, y0)
    assert rel(out.cpu().numpy(), ref) <= 1e-11


@pytest.mark.parametrize('method', list(SOLVERS))
def test_fused_float32_within_its_band(method):
    g = make_g('notebook', 3, dtype=torch.float32)
    s = SOLVERS[method](rhs.Lorenz(), g)
    y0 = y0_for(3, 37)
    out = s.trajectory(torch.tensor(T129, device=DEV), torch.tensor(y0, device=DEV, dtype=torch.float32))
    assert s.last_stats['engine'] == 'fused' and out.dtype == torch.float32
    ref = HR.trajectory(method, HR.lorenz, HR.g_layers(g), T129, y0)
    assert rel(out.double().cpu().numpy(), ref) <= F32_BAND


def test_zero_correction_is_odeint_euler_to_the_bit():
    g = make_g('notebook', 3)
    with torch.no_grad():
        g[-1].weight.zero_()
        g[-1].bias.zero_()
    t = torch.arange(129, dtype=torch.float64, device=DEV) / 128
    y0 = torch.tensor(y0_for(3, 37), device=DEV)
    s = H.HyperEuler(rhs.Lorenz(), g)
    hyp = s.trajectory(t, y0)
    assert s.last_stats['engine'] == 'fused'
    ref = odeint(rhs.Lorenz(), y0, t, method='euler')
    assert torch.equal(hyp, ref)


def test_one_launch_per_call_in_every_mode():
    g = make_g('notebook', 3)
    s = H.HyperEuler(rhs.Lorenz(), g)
    t = torch.tensor(T129, device=DEV)
    y0 = torch.tensor(y0_for(3, 37), device=DEV)
    traj = s.trajectory(t, y0)
    assert (s.last_stats['engine'], s.last_stats['n_launches']) == ('fused', 1), s.last_stats
    r1 = s.residual_trajectory(t, traj)
    assert (s.last_stats['engine'], s.last_stats['n_launches']) == ('fused', 1), s.last_stats
    r2 = s._hypersolver_residuals(t, traj)
    assert (s.last_stats['engine'], s.last_stats['n_launches']) == ('fused', 1), s.last_stats
    assert tuple(r1.shape) == (128, 37, 3) and tuple(r2.shape) == (129, 37, 3)


@pytest.mark.parametrize('fk', ['lorenz', 'vdp_plugin'])
def test_residuals_match_the_restatement(fk):
    mk, d, fnp, opts = F_CASES[fk]
    g = make_g('tanh50', d)
    s = H.HyperEuler(mk(), g, options=opts)
    t = torch.tensor(T129, device=DEV)
    y0 = torch.tensor(y0_for(d, 37), device=DEV)
    traj = s.trajectory(t, y0)
    base = traj.cpu().numpy()
    r1 = s.residual_trajectory(t, traj)
    r2 = s._hypersolver_residuals(t, traj)
    assert rel(r1.cpu().numpy(), HR.residual_trajectory(fnp, T129, base)) <= 1e-11
    assert rel(r2.cpu().numpy(), HR.hypersolver_residuals(fnp, HR.g_layers(g), T129, base)) <= 1e-11
    # on HyperEuler's own trajectory the recovered residuals are g itself (up to the cancellation in base[i+1] - base[i])
    assert rel(r1.cpu().numpy(), r2[:-1].cpu().numpy()) <= 1e-6


def test_weights_edited_in_place_are_seen_no_stale_pack():
    for gk in ('notebook', 'softplus128'):                     # weights in LDS / packed to the workspace
        g = make_g(gk, 3)
        s = H.HyperHeun(rhs.Lorenz(), g)
        t = torch.tensor(T129, device=DEV)
        y0 = torch.tensor(y0_for(3, 37), device=DEV)
        a = s.trajectory(t, y0).clone()
        with torch.no_grad():
            for m in g:
                if isinstance(m, nn.Linear):
                    m.weight.mul_(1.5)
                    m.bias.add_(0.25)
        b = s.trajectory(t, y0)
        assert s.last_stats['engine'] == 'fused'
        assert not torch.allclose(a, b)
        ref = HR.trajectory('heun', HR.lorenz, HR.g_layers(g), T129, y0.cpu().numpy())
        assert rel(b.cpu().numpy(), ref) <= 1e-11
        eager = s._eager(0, t, y0)
        assert rel(b.cpu().numpy(), eager.cpu().numpy()) <= 1e-11


def test_trainable_g_takes_the_eager_engine_and_trains():
    g = make_g('notebook', 3).requires_grad_(True)
    s = H.HyperHeun(rhs.Lorenz(), g)
    t = torch.tensor(T129[:33], device=DEV)
    y0 = torch.tensor(y0_for(3, 16), device=DEV)
    with torch.no_grad():
        fused = s.trajectory(t, y0)
    assert s.last_stats['engine'] == 'fused'
    out = s.trajectory(t, y0)
    assert s.last_stats['engine'] == 'eager' and 'grad' in s.last_stats['why']
    assert rel(out.detach().cpu().numpy(), fused.cpu().numpy()) <= 1e-11
    out.pow(2).mean().backward()
    for p in g.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0


def test_long_heun_on_van_der_pol_fused_against_eager():
    g = make_g('tanh50', 2)
    s = H.HyperHeun(plugin_examples.van_der_pol(5.0), g)
    t = torch.arange(10000, dtype=torch.float64, device=DEV) * 1e-3
    y0 = torch.tensor(y0_for(2, 1), device=DEV)
    fused = s.trajectory(t, y0)
    assert (s.last_stats['engine'], s.last_stats['n_launches']) == ('fused', 1)
    eager = s._eager(0, t, y0)
    assert rel(fused.cpu().numpy(), eager.cpu().numpy()) <= 1e-9


def test_large_batch_runs_in_one_launch():
    g = make_g('notebook', 3)
    s = H.HyperEuler(rhs.Lorenz(), g)
    t = torch.linspace(0., 10., 1001, dtype=torch.float64, device=DEV)
    y0 = torch.tensor(y0_for(3, 65536), device=DEV)
    out = s.trajectory(t, y0)
    assert (s.last_stats['engine'], s.last_stats['n_launches']) == ('fused', 1)
    assert tuple(out.shape) == (1001, 65536, 3) and bool(torch.isfinite(out).all())
