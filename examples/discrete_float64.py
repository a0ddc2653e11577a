"""Exact fixed-grid gradients of a FLOAT64 network in one launch: a training step of ODEBlock(gradient='discrete', solver='rk4') over a
float64 ODEFunc, once with `discrete.MLP64 = 'auto'` (the opt-in float64 fused mlp sweep, csrc/mi_ode_discrete64.h) and once with the
switch off (the generic sweep: one taped re-evaluation and one torch.autograd.grad call per grid interval).  Prints the engine of each
backward, the time of each step and the largest difference between the two sets of gradients, relative to the largest entry.

    python examples/discrete_float64.py [--batch 4096] [--points 5] [--time-dependent]
"""
import argparse
import time

import torch

from tfdiffeq_amd import discrete, models, odeint_discrete


def step(block, x, t, w):
    for p in block.parameters():
        p.grad = None
    xi = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (block(xi, eval_times=t)[-1] * w).sum().backward()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    return [xi.grad] + [p.grad.clone() for p in block.parameters()], dict(odeint_discrete.last_backward_stats), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--points', type=int, default=5)
    ap.add_argument('--time-dependent', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    func = models.ODEFunc(64, 128, time_dependent=args.time_dependent, non_linearity='tanh').double().to(dev)
    block = models.ODEBlock(func, solver='rk4', gradient='discrete')
    x = torch.randn(args.batch, 64, dtype=torch.float64, device=dev)
    w = torch.randn(args.batch, 64, dtype=torch.float64, device=dev)
    t = torch.linspace(0., 1., args.points, dtype=torch.float64)
    results = {}
    for switch in ('auto', False):
        discrete.MLP64 = switch
        step(block, x, t, w)                                 # (the first call creates the engines)
        grads, stats, ms = step(block, x, t, w)
        results[switch] = grads
        print('discrete.MLP64 = %-6r engine: %s, %s launch(es), %.2f ms per training step%s'
              % (switch, stats['engine'], stats['n_launches'], ms, ('; why: ' + stats['why']) if stats['why'] else ''))
    discrete.MLP64 = False
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(results['auto'], results[False]))
    print('largest gradient difference between the two sweeps: %.2e of the largest entry' % worst)


if __name__ == '__main__':
    main()
