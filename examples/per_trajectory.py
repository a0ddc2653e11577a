"""An ensemble of independent Lorenz systems with spread initial conditions, solved both ways.

Shared control (the default, the reference's semantics): the batch is ONE system - one error norm over all rows, one accept decision, one
step size; a row's result depends on which other rows share the call.  options={'per_trajectory': True}: every row is an integration of its
own - row i is exactly what odeint(f, y0[i:i+1], t) returns - and all of them run in one launch (csrc/mi_ode_rows.h).

usage: python examples/per_trajectory.py [--batch 4096]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import odeint, rhs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    y0 = torch.tensor(rng.randn(args.batch, 3) * 10 ** np.linspace(-2, 1.3, args.batch)[:, None], device=dev)
    t = torch.linspace(0., 1., 5, dtype=torch.float64)
    tol = dict(rtol=1e-6, atol=1e-9, method='dopri5')
    print(odeint.plan(rhs.Lorenz(), y0, t, options={'per_trajectory': True}, **tol)['kernel'])

    shared = odeint(rhs.Lorenz(), y0, t, **tol)
    n_shared = odeint.last_stats['n_attempts']
    rows = odeint(rhs.Lorenz(), y0, t, options={'per_trajectory': True}, **tol)
    st = odeint.last_stats
    att = st['rows']['n_attempts'].cpu().numpy()

    print('shared control:         %d attempts for every row (one launch)' % n_shared)
    print('per-trajectory control: %d .. %d attempts per row, mean %.1f (one launch; the call lasts as long as its slowest row: %d)'
          % (att.min(), att.max(), att.mean(), st['n_attempts']))
    print('attempts   rows')
    for n, c in zip(*np.unique(att, return_counts=True)):
        print('%8d   %5d  %s' % (n, c, '#' * max(1, int(60 * c / att.size))))
    one = odeint(rhs.Lorenz(), y0[7:8], t, **tol)
    print('row 7 equals the call on y0[7:8] alone: %s (shared control: %s)'
          % (bool(torch.equal(rows[:, 7], one[:, 0])), bool(torch.equal(shared[:, 7], one[:, 0]))))
    print('largest difference between the two results: %.3e' % float((rows - shared).abs().max()))


if __name__ == '__main__':
    main()
