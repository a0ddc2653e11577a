"""Hypersolvers on the Lorenz system: the workflow of the reference's examples/hyper_solvers.ipynb on this library.

  1. ground truth: Lorenz over t = 0, 0.01, .., 99.99 from odeint dopri5 (rtol = atol = 1e-8), float64, on the GPU
  2. g = Linear(7, 64) PReLU(64) Linear(64, 64) PReLU(64) Linear(64, 64) PReLU(64) Linear(64, 3)
  3. pretraining: 100 batches of 16 one-step problems sampled from the ground truth, Adam, eager autograd (HyperHeun, dt = 0.01)
  4. predict() - the whole 10 000-point trajectory from the first state - and predict_with_ground_truth_states() - one step from
     every ground-truth state - on the fused engine (one launch each)
  5. the mean squared errors and the wall times

    python examples/hyper_solvers.py
"""
import os
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import hyper_solvers, odeint, rhs  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    dev = torch.device('cuda:0')
    dt = torch.float64
    f = rhs.Lorenz()
    t = torch.arange(0, 100, 0.01, dtype=dt, device=dev)
    y0 = torch.tensor([[1., 1., 1.]], dtype=dt, device=dev)
    truth, t_gt = timed(lambda: odeint(f, y0, t, rtol=1e-8, atol=1e-8, method='dopri5')[:, 0])       # [T, 3]

    torch.manual_seed(0)
    g = nn.Sequential(nn.Linear(7, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64),
                      nn.Linear(64, 3)).to(device=dev, dtype=dt)
    solver = hyper_solvers.HyperHeun(f, g)
    opt = torch.optim.Adam(g.parameters(), lr=1e-3)
    step_t = t[:2]

    def pretrain():
        gen = torch.Generator().manual_seed(1)
        loss = None
        for _ in range(100):
            idx = torch.randint(0, t.shape[0] - 1, (16,), generator=gen).to(dev)
            pred = solver.trajectory(step_t, truth[idx])[-1]              # one step from each sampled state (eager engine: g trains)
            loss = (pred - truth[idx + 1]).pow(2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
        return float(loss)
    last_loss, t_train = timed(pretrain)
    train_engine = dict(solver.last_stats)

    def predict():
        with torch.no_grad():
            return solver.trajectory(t, truth[:1])[:, 0]

    def predict_with_ground_truth_states():
        with torch.no_grad():
            return solver.trajectory(step_t, truth[:-1])[-1]
    predict()                                                             # (first call: code object load)
    traj, t_pred = timed(predict)
    pred_stats = dict(solver.last_stats)
    predict_with_ground_truth_states()
    onestep, t_gts = timed(predict_with_ground_truth_states)
    gts_stats = dict(solver.last_stats)

    print('ground truth (odeint dopri5, rtol = atol = 1e-8, %d points): %.3f s' % (t.shape[0], t_gt))
    print('pretraining: 100 batches of 16, Adam, engine %s: %.3f s, last batch loss %.3e' % (train_engine['engine'], t_train, last_loss))
    print('predict(): HyperHeun over %d points from the first state, engine %s, %s launch(es): %.4f s, MSE %.4e (chaotic: the '
          'long-horizon error saturates at the attractor scale)' % (t.shape[0], pred_stats['engine'], pred_stats['n_launches'], t_pred,
                                                                     float((traj - truth).pow(2).mean())))
    print('predict_with_ground_truth_states(): one step from each of %d states, engine %s, %s launch(es): %.4f s, one-step MSE %.4e'
          % (t.shape[0] - 1, gts_stats['engine'], gts_stats['n_launches'], t_gts, float((onestep - truth[1:]).pow(2).mean())))
    with torch.no_grad():
        for m in g:
            if isinstance(m, nn.Linear) and m is g[-1]:
                m.weight.zero_()
                m.bias.zero_()
        plain = solver.trajectory(step_t, truth[:-1])[-1]
    print('for comparison, Heun without the correction (g = 0): one-step MSE %.4e' % float((plain - truth[1:]).pow(2).mean()))


if __name__ == '__main__':
    main()
