"""One ODEFunc network evaluated over a batch whose rows differ in scale, solved both ways.

Shared control (the default, the reference's semantics): the batch is ONE system - one error norm over all rows, one step size; a sample's
result depends on which other samples share its batch.  options={'per_trajectory': True}: every row is an integration of its own, on the
matrix cores - a 32-row tile per workgroup with the weights resident, every row of the tile with its own step, error record, controller
and output cursor (csrc/mi_ode_rows_mlp.h) - all in one launch.  Re-slicing or re-ordering the batch changes no bit of any row.

usage: python examples/per_trajectory_mlp.py [--batch 4096]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import models, odeint  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    func = models.ODEFunc(16, 64, non_linearity='tanh').to(dev)                 # 16 -> 64 -> 64 -> 16
    gen = torch.Generator().manual_seed(1)
    scale = torch.logspace(-1.0, 1.0, args.batch)[torch.randperm(args.batch, generator=gen)]
    y0 = (torch.randn(args.batch, 16, generator=gen) * scale[:, None]).to(dev)
    t = torch.linspace(0., 2., 5, dtype=torch.float64)
    tol = dict(rtol=1e-4, atol=1e-6, method='dopri5')
    f = func.device_rhs()                                                       # the network's fused descriptor (an rhs.MLP)
    print(odeint.plan(f, y0, t, options={'per_trajectory': True}, **tol)['kernel'])

    with torch.no_grad():
        shared = odeint(f, y0, t, **tol)
        n_shared = odeint.last_stats['n_attempts']
        rows = odeint(f, y0, t, options={'per_trajectory': True}, **tol)
        st = odeint.last_stats
        att = st['rows']['n_attempts'].cpu().numpy()
        print('shared control:         %d attempts for every row (one launch, a grid hand-off per attempt)' % n_shared)
        print('per-trajectory control: %d .. %d attempts per row, mean %.1f (one launch, no hand-off; a tile lasts as long as its slowest row)'
              % (att.min(), att.max(), att.mean()))
        print('attempts   rows')
        for n, c in zip(*np.unique(att, return_counts=True)):
            print('%8d   %5d  %s' % (n, c, '#' * max(1, int(60 * c / att.size))))
        half = odeint(f, y0[: args.batch // 2].contiguous(), t, options={'per_trajectory': True}, **tol)
        half_shared = odeint(f, y0[: args.batch // 2].contiguous(), t, **tol)
    print('the first half of the batch solved alone changes no bit of its rows: %s (shared control: %s)'
          % (bool(torch.equal(half, rows[:, : args.batch // 2])), bool(torch.equal(half_shared, shared[:, : args.batch // 2]))))
    print('largest difference between the two results: %.3e' % float((rows - shared).abs().max()))


if __name__ == '__main__':
    main()
