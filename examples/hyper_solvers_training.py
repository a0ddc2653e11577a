"""Training a hypersolver on the fused engine: cells 15 and 17 of the reference's examples/hyper_solvers.ipynb on this library.

  1. ground truth: Lorenz over t = 0, 0.01, .. from odeint dopri5 (rtol = atol = 1e-8), float64, on the GPU
  2. g = Linear(7, 64) PReLU(64) Linear(64, 64) PReLU(64) Linear(64, 64) PReLU(64) Linear(64, 3); HyperHeun(f, g, options={'grad': 'auto'})
  3. cell 15, pretraining: 100 optimizer steps on the 16-point trajectory from the initial state against the first 16 ground-truth states
  4. cell 17, training: 16-point trajectories from the ground-truth state at the start of each window, Adam on a cosine schedule with
     gradient-norm clipping, --epochs passes over the windows (the notebook: 20 epochs of 625 windows)
  5. the engines of the forward and the backward (`last_stats`, `last_backward_stats`: one launch each, two when g's weight images do
     not fit in LDS), the loss curve and the wall time per optimizer step

    python examples/hyper_solvers_training.py [--epochs 1] [--points 2000] [--grad auto|off]
"""
import argparse
import math
import os
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import hyper_solvers, odeint, rhs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=1)
    ap.add_argument('--points', type=int, default=2000)
    ap.add_argument('--grad', choices=['auto', 'off'], default='auto')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    dt = torch.float64
    f = rhs.Lorenz()
    t = torch.arange(args.points, dtype=dt, device=dev) * 0.01
    y0 = torch.tensor([[1., 1., 1.]], dtype=dt, device=dev)
    truth = odeint(f, y0, t, rtol=1e-8, atol=1e-8, method='dopri5')[:, 0]                  # [T, 3]

    torch.manual_seed(0)
    g = nn.Sequential(nn.Linear(7, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64),
                      nn.Linear(64, 3)).to(device=dev, dtype=dt)
    solver = hyper_solvers.HyperHeun(f, g, options={'grad': 'auto' if args.grad == 'auto' else False})
    batch = 16

    def train_step(opt, t_win, init, target, clip=None):
        pred = solver.trajectory(t_win, init)[:, 0]                                            # [16, 3]
        loss = (target - pred).pow(2).sum()
        opt.zero_grad()
        loss.backward()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(g.parameters(), clip)
        opt.step()
        return loss.detach()

    # cell 15
    opt = torch.optim.Adam(g.parameters(), lr=0.01)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    curve = []
    for idx in range(100):
        loss = train_step(opt, t[:batch], y0, truth[:batch])
        if (idx + 1) % 10 == 0:
            curve.append(float(loss))
    torch.cuda.synchronize()
    t_pre = time.perf_counter() - t0
    print('forward: engine %s (%s), %s launch(es)' % (solver.last_stats['engine'], solver.last_stats['why'], solver.last_stats['n_launches']))
    print('backward: %s' % (solver.last_backward_stats or 'torch autograd through the eager loop'))
    print('pretraining (cell 15): 100 optimizer steps in %.3f s (%.2f ms per step); loss every 10 steps: %s'
          % (t_pre, 10 * t_pre, ' '.join('%.3e' % v for v in curve)))

    # cell 17
    windows = args.points // batch
    total = windows * args.epochs
    opt = torch.optim.Adam(g.parameters(), lr=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: (1 - 1e-4) * 0.5 * (1 + math.cos(math.pi * min(k, total) / total)) + 1e-4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for epoch in range(args.epochs):
        losses = []
        for w in range(windows):
            lo = w * batch
            losses.append(train_step(opt, t[lo:lo + batch], truth[lo:lo + 1], truth[lo:lo + batch], clip=10.0))
            sched.step()
        print('epoch %d: mean loss over %d windows %.4e' % (epoch + 1, windows, float(torch.stack(losses).detach().mean())))
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    print('training (cell 17): %d optimizer steps in %.3f s (%.2f ms per step), forward engine %s, backward engine %s'
          % (total, t_train, 1e3 * t_train / total, solver.last_stats['engine'], solver.last_backward_stats.get('engine', 'autograd')))


if __name__ == '__main__':
    main()
