"""Fit sigma, rho, beta of the Lorenz system to the noisy end states of an ensemble - every member solved, and differentiated, on its own.

odeint_adjoint(module, y0, t, options={'per_trajectory': True}): the forward is the per-trajectory solve (every row its own step control,
one launch, csrc/mi_ode_rows.h); the backward applies the adjoint method to every trajectory alone - its own augmented state
(y, adj_y, adj_t, adj_params), its own per-component step control - for all rows in ONE launch (csrc/mi_ode_rows_adjoint.h) behind a vjp
generated from the module's trace.  `odeint_adjoint.last_backward_stats['rows']` holds the per-member pieces: d loss / d theta of every
member ([batch, 3]), its time vjps, its attempt counts.

usage: python examples/per_trajectory_gradients.py [--batch 512] [--steps 150]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import odeint, odeint_adjoint  # noqa: E402


class Lorenz(torch.nn.Module):
    def __init__(self, sigma, rho, beta, device):
        super(Lorenz, self).__init__()
        self.sigma, self.rho, self.beta = (torch.nn.Parameter(torch.tensor(v, dtype=torch.float64, device=device)) for v in (sigma, rho, beta))

    def forward(self, t, y):
        x, u, z = y[..., 0], y[..., 1], y[..., 2]
        return torch.stack([self.sigma * (u - x), x * (self.rho - z) - u, x * u - self.beta * z], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--steps', type=int, default=150)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    y0 = (torch.tensor([1., 1., 1.], dtype=torch.float64) + torch.randn(args.batch, 3, generator=g, dtype=torch.float64)).to(dev)
    t = torch.tensor([0., 0.4], dtype=torch.float64)
    tol = dict(rtol=1e-6, atol=1e-9, method='dopri5', options={'per_trajectory': True})
    truth = Lorenz(10., 28., 8. / 3., dev)
    with torch.no_grad():
        target = odeint(truth, y0, t, **tol)[-1]
        target = target + 0.01 * torch.randn(target.shape, generator=g, dtype=torch.float64).to(dev)

    model = Lorenz(8., 25., 2., dev)
    print(odeint_adjoint.plan(model, y0, t, **tol)['kernel'])
    opt = torch.optim.Adam(model.parameters(), lr=0.1)
    for step in range(args.steps + 1):
        opt.zero_grad()
        end = odeint_adjoint(model, y0, t, **tol)[-1]
        loss = (end - target).pow(2).mean()
        loss.backward()
        if step % 25 == 0:
            st = odeint_adjoint.last_backward_stats
            att = st['rows']['n_attempts'].sum(dim=1)
            print('step %3d  loss %.3e  sigma %.4f rho %.4f beta %.4f   backward: %d launch, %d .. %d attempts per member'
                  % (step, loss.item(), model.sigma.item(), model.rho.item(), model.beta.item(), st['n_launches'], int(att.min()), int(att.max())))
        opt.step()
    rows = odeint_adjoint.last_backward_stats['rows']
    spread = rows['grad_params'].abs().max(dim=0).values
    print('per-member sensitivities |d loss / d (sigma, rho, beta)|, largest member: %.2e %.2e %.2e' % tuple(float(v) for v in spread))
    print('recovered sigma %.3f (10), rho %.3f (28), beta %.3f (2.667)' % (model.sigma.item(), model.rho.item(), model.beta.item()))


if __name__ == '__main__':
    main()
