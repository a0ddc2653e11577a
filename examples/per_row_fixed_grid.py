"""Ragged observations, one launch in each direction: an rk4 fit of a small trainable callable on every series' own observation times.

Each of the 512 series was observed at its own times (4 .. 12 of them on [0, 1]; states of size <= 0.71, so that every rk4 step stays
bounded); `t` is [batch, T] with NaN padding and options['t_lengths'] says how
many times of a row count.  `odeint_discrete` solves every row on its own grid (csrc/mi_ode_fixed_rows_t.h) and returns the exact gradient
of every row's own discrete map (csrc/mi_ode_discrete_row_t.h); the padding of the solution is exactly 0 and takes no part in the loss.

usage: python examples/per_row_fixed_grid.py [--iters 200]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import odeint, odeint_discrete          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    args = ap.parse_args()
    dev, B, T = torch.device('cuda:0'), 512, 12
    rng = np.random.default_rng(0)
    lengths = rng.integers(4, T + 1, size=B).astype(np.int32)
    t = np.full((B, T), np.nan)
    for i, n in enumerate(lengths):
        t[i, :n] = np.concatenate([[0.], np.sort(rng.uniform(0.05, 1.0, size=n - 1))])
    t, ln = torch.as_tensor(t, device=dev), torch.as_tensor(lengths, device=dev)
    mask = (torch.arange(T, device=dev)[:, None] < ln[None, :])[:, :, None]
    y0 = torch.as_tensor(rng.uniform(-0.5, 0.5, size=(B, 2)), device=dev)
    A_true = torch.tensor([[-0.1, 2.0], [-2.0, -0.1]], dtype=torch.float64, device=dev)
    with torch.no_grad():                                   # the observations: the same map with the true matrix
        obs = odeint(lambda t_, y: (y ** 3) @ A_true, y0, t, method='rk4', options={'t_lengths': ln})
    A = torch.zeros(2, 2, dtype=torch.float64, device=dev, requires_grad=True)
    opt = torch.optim.Adam([A], lr=0.05)

    def f(t_, y):                                            # (one callable for the whole fit: traced and compiled once)
        return (y ** 3) @ A
    for it in range(args.iters):
        opt.zero_grad()
        sol = odeint_discrete(f, y0, t, method='rk4', options={'t_lengths': ln})
        loss = ((sol - obs) ** 2 * mask).sum() / mask.sum()
        loss.backward()
        opt.step()
        if it % 50 == 0 or it == args.iters - 1:
            print('iter %4d  loss %.3e  |A - A_true| %.3e  backward: %s' % (it, float(loss), float((A - A_true).abs().max()),
                                                                            odeint_discrete.last_backward_stats['engine']))


if __name__ == '__main__':
    main()
