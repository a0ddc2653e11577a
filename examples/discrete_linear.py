"""Training a linear system y' = y W + b with the exact gradient of the fixed-grid solve, the whole backward in one launch.

`odeint_discrete(..., linear='auto')` hands models.LinearODEFunc (and callables such as `lambda t, y: y @ W`) to the fused linear sweep
(csrc/mi_ode_discrete_linear.h); `discrete.LINEAR = 'auto'` does the same for ODEBlock / ODENet(gradient='discrete').

usage: python examples/discrete_linear.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfdiffeq_amd import models, odeint, odeint_discrete, rhs  # noqa: E402


def main():
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    dim, batch = 16, 512
    true_A = -0.5 * torch.eye(dim, dtype=torch.float64) + 0.4 * torch.randn(dim, dim, dtype=torch.float64) / dim ** 0.5
    t = torch.linspace(0., 1., 9, dtype=torch.float64)
    y0 = torch.randn(batch, dim, dtype=torch.float64, device=dev)
    with torch.no_grad():
        target = odeint(rhs.Linear(true_A.to(dev)), y0, t, method='rk4')
    func = models.LinearODEFunc(dim, bias=True).to(dev)
    opt = torch.optim.Adam(func.parameters(), lr=2e-2)
    for it in range(200):
        opt.zero_grad()
        sol = odeint_discrete(func, y0, t, method='rk4', linear='auto')
        loss = (sol - target).pow(2).mean()
        loss.backward()
        opt.step()
        if it % 50 == 0 or it == 199:
            st = odeint_discrete.last_backward_stats
            print('step %3d  loss %.3e  backward: %s, %d launch(es)' % (it, float(loss), st['engine'], st['n_launches']))
    print('max |W - A| = %.3e' % float((func.weight.detach().cpu() - true_A).abs().max()))


if __name__ == '__main__':
    main()
