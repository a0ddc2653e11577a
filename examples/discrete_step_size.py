"""An ODEBlock over [0, 1] that takes 16 rk4 steps instead of one, trained with the exact gradient of that solve.

`block.options = {'step_size': 1 / 16}` gives the fixed-grid solver a grid of its own; with `discrete.OWN_GRID = True` (or
`odeint_discrete(..., own_grid=True)`) the block's gradient='discrete' branch accepts it: the forward is one launch that walks the grid
and returns y(1), the backward recomputes the 17 grid states and runs the fused sweep over them.  The gradient is compared with autograd
through the taped restatement of the same solve (tests/discrete_grid_restatement.py, float64 on the CPU).

usage: python examples/discrete_step_size.py      (from a source checkout: the comparison imports the restatements under tests/)
"""
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfdiffeq_amd import discrete, models, odeint_discrete  # noqa: E402
from tests import discrete_grid_restatement as DGR  # noqa: E402
from tests import discrete_restatement as DR  # noqa: E402


def main():
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    func = models.ODEFunc(4, 16, non_linearity='tanh').to(dev)
    block = models.ODEBlock(func, solver='rk4', gradient='discrete')
    block.options = {'step_size': 1 / 16}
    discrete.OWN_GRID = True
    x = torch.randn(256, 4, device=dev)
    target = torch.roll(x, 1, dims=1)

    # the gradient of one step against the taped restatement
    loss = (block(x) - target).pow(2).mean()
    loss.backward()
    st = odeint_discrete.last_backward_stats
    print('backward: %s over %d grid steps, %s launch(es), own grid %s' % (st['engine'], st['n_steps'], st['n_launches'], st['own_grid']))
    f64 = copy.deepcopy(func).double().cpu()
    y0 = x.double().cpu().requires_grad_(True)
    sol = DGR.solve(f64, y0, torch.tensor([0., 1.]), 'rk4', 1 / 16, time_dtype=torch.float32)
    (sol[-1] - target.double().cpu()).pow(2).mean().backward()
    for (name, p), q in zip(func.named_parameters(), f64.parameters()):
        print('  %-10s max|got - taped| / max|taped| = %.2e (ceiling %.2e)' % (name, DR.rel_max(p.grad, q.grad), DR.ceiling32(16, 'rk4')))

    opt = torch.optim.Adam(func.parameters(), lr=1e-2)
    for it in range(100):
        opt.zero_grad()
        loss = (block(x) - target).pow(2).mean()
        loss.backward()
        opt.step()
        if it % 25 == 0 or it == 99:
            print('step %3d  loss %.3e' % (it, float(loss)))


if __name__ == '__main__':
    main()
