"""A full training step (forward + loss on y(1) + backward) of models.LinearODEFunc over t = [0, 1] with 32 rk4 steps and the gradient of
the discrete map, three ways, at 65536 x 128 float64 (config 4's shape) and 4096 x 128 float32:

  stored   what odeint_discrete could do before options['step_size'] was accepted: all 33 grid times passed as `t`, linear='auto' - [33, batch,
           dim] returned, as many cotangents kept, the default-grid linear sweep streams both;
  recompute  own_grid=True with discrete.GRID_KERNEL = False: t = [0, 1], options = {'step_size': 1 / 32}; the backward recomputes the 33 grid
           states in one launch and runs the same default-grid linear sweep;
  kernel   own_grid=True, discrete.GRID_KERNEL = True: the one-launch kernel that recomputes its checkpoints into a scratch that does not
           depend on the batch (csrc/mi_ode_discrete_linear.h, GRID = true).

One process, in-run HIP events, min / median / max over the timed steps after the warm-up.  Memory: torch.cuda.max_memory_allocated() over
the timed steps (reset after the warm-up) plus the scratch the own-grid engine allocated outside torch's allocator.

usage: python scripts/bench_discrete_grid.py [--steps 20] [--warmup 5] [--out profiles/discrete_grid_bench.txt] [--only kernel]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tfdiffeq_amd import discrete, models, odeint_discrete  # noqa: E402

SHAPES = ((65536, 128, torch.float64), (4096, 128, torch.float32))
N_STEPS = 32


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), statistics.median(ms), max(ms), torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'discrete_grid_bench.txt'))
    ap.add_argument('--only', default='', help='comma-separated subset of stored,recompute,kernel')
    args = ap.parse_args()
    only = set(filter(None, args.only.split(',')))
    dev = torch.device('cuda:0')
    lines = ['# scripts/bench_discrete_grid.py --steps %d --warmup %d: %s, models.LinearODEFunc with bias, rk4, t = [0, 1], %d grid steps, loss on y(1); '
             'ms per training step (min / median / max), peak bytes of the step (torch allocator + engine scratch)'
             % (args.steps, args.warmup, torch.cuda.get_device_name(0), N_STEPS)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for batch, dim, dtype in SHAPES:
        torch.manual_seed(0)
        func = models.LinearODEFunc(dim, bias=True, dtype=dtype).to(dev)
        x = torch.randn(batch, dim, device=dev, dtype=dtype)
        w = torch.randn(batch, dim, device=dev, dtype=dtype)
        t_all = torch.linspace(0., 1., N_STEPS + 1, dtype=dtype)
        t_ends = torch.tensor([0., 1.], dtype=dtype)
        opts = {'step_size': 1.0 / N_STEPS}

        def step(**kw):
            for p in func.parameters():
                p.grad = None
            xi = x.clone().requires_grad_(True)
            (odeint_discrete(func, xi, method='rk4', linear='auto', **kw)[-1] * w).sum().backward()

        head = '%5d x %3d %s' % (batch, dim, str(dtype).replace('torch.', ''))
        grads = {}
        for name, kernel, kw, engine in (('stored', True, dict(t=t_all), 'fused linear sweep'),
                                         ('recompute', False, dict(t=t_ends, options=opts, own_grid=True), 'fused linear sweep'),
                                         ('kernel', True, dict(t=t_ends, options=opts, own_grid=True), 'fused linear sweep (own grid)')):
            if only and name not in only:
                continue
            discrete.clear_engines()
            torch.cuda.empty_cache()
            discrete.GRID_KERNEL = kernel
            lo, med, hi, peak = timed(lambda: step(**kw), args.steps, args.warmup)
            st = odeint_discrete.last_backward_stats
            assert st['engine'] == engine and st['n_steps'] == N_STEPS, st
            scratch = 0
            if name == 'kernel':
                scratch = st['own_grid']['scratch_bytes']
            grads[name] = func.weight.grad.detach().clone()
            say('%s  %-9s %-30s %9.3f / %9.3f / %9.3f ms   peak %7.3f GB (allocator %.3f + engine scratch %.3f)  launches: backward %s, recompute %s'
                % (head, name, st['engine'], lo, med, hi, (peak + scratch) / 1e9, peak / 1e9, scratch / 1e9, st['n_launches'],
                   st.get('own_grid', {}).get('recompute_launches', '-')))
        discrete.GRID_KERNEL = True
        if 'stored' in grads:
            for name in ('recompute', 'kernel'):
                if name in grads:
                    d = float((grads[name] - grads['stored']).abs().max() / grads['stored'].abs().max())
                    say('%s  %-9s weight gradient against stored: max|diff| / max|ref| = %.3e' % (head, name, d))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
