"""What per-row time grids cost on a fixed grid: k_fixed_rowlocal / k_discrete_rowlocal (shared `t`) against k_fixed_rowlocal_t /
k_discrete_rowlocal_t (a 2-D `t`; csrc/mi_ode_fixed_rows_t.h, csrc/mi_ode_discrete_row_t.h) on the same inputs.

Shape: 65 536 Lorenz systems (forward) and the `tanh8` callable of tests/discrete_lowered_cases.py (forward + backward through
odeint_discrete, loss = sum of the solution), rk4, T = 16 on [0, 0.5].  Lines per system and dtype:
  (a) shared t        the one-launch call that existed before: t [T]
  (b) replicated t    the new kernels fed the same times, one copy per row - the whole call, validation of `t` included
  (b') ... prepared   the same with `t` validated once outside the timed region (fixed_rows.times + the solver's integrate_rows_t;
                      forward only): (b') / (a) is what per-lane times cost the kernel, (b) - (b') what the validation costs
  (c) ragged lengths  the new kernels, lengths cycling through 1 .. T (NaN padding), with the share of lane-steps that are idle
                      (a wavefront runs until its longest row ends)
ms per call from in-run HIP events: min / median / max of the timed calls after the warm-up.  --tree PATH imports the package from
another checkout (line (a) only exists there if it predates the feature: --only-a), so that the same script times the parent commit
in the same visit.

usage: python scripts/bench_per_row_fixed.py [--steps 20] [--warmup 5] [--batch 65536] [--tree PATH] [--only-a] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16
END = 0.5


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


def idle_share(lengths):
    """Share of the lane-steps of the wavefronts' loops in which a lane has no step of its own (64 consecutive rows per wavefront)."""
    steps = np.asarray(lengths, dtype=np.int64) - 1
    pad = (-len(steps)) % 64
    w = np.concatenate([steps, np.zeros(pad, dtype=np.int64)]).reshape(-1, 64)
    total = int((w.max(axis=1) * 64).sum())
    return 1.0 - float(steps.sum()) / max(total, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--only-a', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, 'tests'))
    import discrete_lowered_cases as DC
    import tfdiffeq_amd
    from tfdiffeq_amd import odeint, odeint_discrete, rhs
    assert os.path.abspath(tfdiffeq_amd.__file__).startswith(tree), tfdiffeq_amd.__file__
    dev = torch.device('cuda:0')
    B = args.batch
    lines = ['# scripts/bench_per_row_fixed.py --steps %d --warmup %d --batch %d%s (tree: %s): %s; rk4, T = %d; ms per call min / median / max'
             % (args.steps, args.warmup, B, ' --only-a' if args.only_a else '', os.path.relpath(tree, ROOT), torch.cuda.get_device_name(0), T)]

    def say(what, r, extra=''):
        lines.append('%-58s %8.4f %8.4f %8.4f%s' % (what, r[0], r[1], r[2], extra))
        print(lines[-1], flush=True)
    t1 = torch.linspace(0., END, T, dtype=torch.float64)
    t2 = t1[None, :].repeat(B, 1).to(dev)                   # (the per-row inputs live on the device, as a training loop keeps them)
    lengths = (1 + np.arange(B) % T).astype(np.int32)
    tr = np.full((B, T), np.nan)
    for i, n in enumerate(lengths):
        tr[i, :n] = np.linspace(0., END, T)[:n]
    tr, ln = torch.as_tensor(tr).to(dev), torch.as_tensor(lengths).to(dev)
    idle = ', idle lane-steps %.1f %%' % (100 * idle_share(lengths))
    for dtype in (torch.float64, torch.float32):
        name = str(dtype).replace('torch.', '')
        y0 = (torch.tensor([1., 1., 1.], dtype=torch.float64) + 0.1 * torch.randn(B, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)).to(dev, dtype)
        f = rhs.Lorenz()
        say('lorenz %s forward (a) shared t' % name, timed(lambda: odeint(f, y0, t1, method='rk4'), args.steps, args.warmup))
        if not args.only_a:
            say('lorenz %s forward (b) replicated t, whole call' % name, timed(lambda: odeint(f, y0, t2, method='rk4'), args.steps, args.warmup))
            from tfdiffeq_amd import fixed_rows
            from tfdiffeq_amd.misc import _check_inputs
            from tfdiffeq_amd.odeint import SOLVERS
            rt = fixed_rows.times(y0, t2, None)
            _ti, fn, st, _ = _check_inputs(f, y0, [0., 1.])
            solver = SOLVERS['rk4'](fn, st)
            say("lorenz %s forward (b') replicated t, t prepared once" % name, timed(lambda: solver.integrate_rows_t(rt), args.steps, args.warmup))
            say('lorenz %s forward (c) ragged lengths' % name, timed(lambda: odeint(f, y0, tr, method='rk4', options={'t_lengths': ln}), args.steps, args.warmup), idle)
        g, params, z0 = DC.tanh8(dev, dtype, 0, batch=B)

        def train(t_, opts=None, lower=None):
            for p in params:
                p.grad = None
            z = z0.clone().requires_grad_(True)
            sol = odeint_discrete(g, z, t_, method='rk4', options=opts, lower=lower)
            sol.sum().backward()
        say('tanh8 %s forward + backward (a) shared t' % name, timed(lambda: train(t1, {'lower': True}, True), args.steps, args.warmup))
        if not args.only_a:
            say('tanh8 %s forward + backward (b) replicated t' % name, timed(lambda: train(t2), args.steps, args.warmup))
            say('tanh8 %s forward + backward (c) ragged lengths' % name, timed(lambda: train(tr, {'t_lengths': ln}), args.steps, args.warmup), idle)
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
