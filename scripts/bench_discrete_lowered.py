"""A full training step (forward + loss + backward) through `odeint_discrete` for lowered Python callables, three ways:

  taped    the solver loop written in torch ops and back-propagated (tests/discrete_restatement.py);
  generic  odeint_discrete(lower=False): fused forward, one taped step + one torch.autograd.grad call per grid interval backward;
  fused    odeint_discrete(lower=True): fused forward, the whole backward in one launch (csrc/mi_ode_discrete_row.h, generated vjp).

Cases: the demo network Sequential(Linear(2, 50), Tanh, Linear(50, 2)) on y ** 3 (P = 252 trainable elements) on the state [20, 1, 2] and
at batch 4096; the dim-8 system tanh(y @ A + b) - 0.5 y (P = 72) at batch 4096 and 65536; rk4 on 5 and 21 grid points, one-step Euler.
One process, in-run HIP events, min / median / max over the timed steps after the warm-up.

usage: python scripts/bench_discrete_lowered.py [--steps 20] [--warmup 5] [--out profiles/discrete_lowered_bench.txt] [--only fused,generic]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import discrete_lowered_cases as DC  # noqa: E402
from tfdiffeq_amd import odeint_discrete  # noqa: E402
from tests import discrete_restatement as DR  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), statistics.median(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'discrete_lowered_bench.txt'))
    ap.add_argument('--only', default='', help='comma-separated subset of taped,generic,fused')
    ap.add_argument('--dtype', default='float32')
    args = ap.parse_args()
    only = set(filter(None, args.only.split(',')))
    dev = torch.device('cuda:0')
    dtype = getattr(torch, args.dtype)
    lines = ['# scripts/bench_discrete_lowered.py --steps %d --warmup %d --dtype %s: %s; ms per training step (min / median / max)'
             % (args.steps, args.warmup, args.dtype, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cases = [('demo net 20x1x2    ', lambda: DC.demo_net(dev, dtype)),
             ('demo net batch 4096', lambda: DC.demo_net(dev, dtype, state=(4096, 2))),
             ('dim-8 batch 4096   ', lambda: DC.tanh8(dev, dtype, batch=4096)),
             ('dim-8 batch 65536  ', lambda: DC.tanh8(dev, dtype, batch=65536))]
    for label, make in cases:
        f, params, y0 = make()
        w = torch.randn_like(y0)
        for method, n in (('rk4', 5), ('rk4', 21), ('euler', 2)):
            t = torch.linspace(0., 1., n, dtype=dtype)

            def step(solve):
                for p in params:
                    p.grad = None
                y = y0.clone().requires_grad_(True)
                (solve(y)[-1] * w).sum().backward()

            head = '%s %-5s N=%2d' % (label, method, n)
            if not only or 'taped' in only:
                say('%s  taped torch loop        %9.3f / %9.3f / %9.3f' % ((head,) + timed(lambda: step(lambda y: DR.solve(f, y, t, method)), args.steps, args.warmup)))
            if not only or 'generic' in only:
                res = timed(lambda: step(lambda y: odeint_discrete(f, y, t, method=method, lower=False)), args.steps, args.warmup)
                assert odeint_discrete.last_backward_stats['engine'] == 'generic sweep'
                say('%s  generic sweep           %9.3f / %9.3f / %9.3f' % ((head,) + res))
            if not only or 'fused' in only:
                res = timed(lambda: step(lambda y: odeint_discrete(f, y, t, method=method, lower=True)), args.steps, args.warmup)
                st = odeint_discrete.last_backward_stats
                assert st['engine'] == 'fused row-local sweep' and st['n_launches'] == 1, st
                say('%s  fused row-local sweep   %9.3f / %9.3f / %9.3f   (P = %d)' % ((head,) + res + (st['n_params'],)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
