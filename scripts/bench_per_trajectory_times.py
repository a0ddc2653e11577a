"""What per-lane output times cost: k_rows_rowlocal (shared `t`) against k_rows_rowlocal_t (a 2-D `t`; csrc/mi_ode_rows_t.h) on the same inputs.

Shape: 65 536 Lorenz systems, rtol 1e-6, atol 1e-9 (float32: 1e-4, 1e-6), dopri5, the two sets of initial conditions of
scripts/bench_per_trajectory.py (`bench`: every row needs about the same steps; `spread`: the tests' 70 rows over 3.3 decades, tiled).
Three lines per input and dtype:
  (a) shared t      options={'per_trajectory': True} with t = [0, 1]: the kernel that existed before
  (b) replicated t  the new kernel fed the same times, one copy per row: (b) / (a) is what per-lane times cost
  (c) own horizons  the new kernel, row i integrates to its own end drawn uniformly from [0.5, 1.5] (seed 2); with the share of the
                    loop the lanes of a wavefront sit idle (a wavefront runs until its slowest lane ends)
ms per call from in-run HIP events: min / median / max of the timed calls after the warm-up.  --tree PATH imports the package from
another checkout (line (a) only exists there if it predates the feature: --only-a), so that the same script times the parent commit in
the same visit.

usage: python scripts/bench_per_trajectory_times.py [--steps 20] [--warmup 5] [--batch 65536] [--tree PATH] [--only-a] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--only-a', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, 'tests'))
    import per_trajectory_cases as PC
    import tfdiffeq_amd
    from tfdiffeq_amd import odeint, rhs
    assert os.path.abspath(tfdiffeq_amd.__file__).startswith(tree), tfdiffeq_amd.__file__
    dev = torch.device('cuda:0')
    lines = ['# scripts/bench_per_trajectory_times.py --steps %d --warmup %d --batch %d%s (tree: %s): %s; Lorenz, dopri5; ms per call min / median / max'
             % (args.steps, args.warmup, args.batch, ' --only-a' if args.only_a else '', os.path.relpath(tree, ROOT), torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    inputs = {'bench ': torch.tensor(np.array([1., 1., 1.]) + 1e-3 * rng.standard_normal((args.batch, 3))),
              'spread': PC.base_y0().repeat(-(-args.batch // 70), 1)[:args.batch].contiguous()}
    t1 = torch.tensor([0., 1.], dtype=torch.float64)
    t_rep = t1[None, :].repeat(args.batch, 1).to(dev)
    ends = torch.tensor(np.random.default_rng(2).uniform(0.5, 1.5, args.batch))
    t_own = torch.stack([torch.zeros_like(ends), ends], dim=1).to(dev)
    f = rhs.Lorenz()
    on = {'per_trajectory': True}

    def idle(att):
        per_wave = att[:att.numel() // 64 * 64].reshape(-1, 64)
        slow = float(per_wave.max(dim=1).values.mean())
        return float(per_wave.mean()), slow, 100.0 * (1.0 - float(per_wave.mean()) / slow)

    for label, y64 in inputs.items():
        for dtype, tol in ((torch.float64, dict(rtol=1e-6, atol=1e-9)), (torch.float32, dict(rtol=1e-4, atol=1e-6))):
            y0 = y64.to(device=dev, dtype=dtype)
            head = 'y0 %s %-7s' % (label, str(dtype).replace('torch.', ''))
            cases = [('(a) shared t     ', t1, 'k_rows_rowlocal:')]
            if not args.only_a:
                cases += [('(b) replicated t ', t_rep, 'k_rows_rowlocal_t:'), ('(c) own horizons ', t_own, 'k_rows_rowlocal_t:'),
                          ('(a) shared t again', t1, 'k_rows_rowlocal:')]
            for name, t, kernel in cases:
                res = timed(lambda: odeint(f, y0, t, method='dopri5', options=on, **tol), args.steps, args.warmup)
                st = dict(odeint.last_stats)
                assert st['per_trajectory'] is True and st['n_launches'] == 1 and st['engine'].startswith(kernel), st
                att = st['rows']['n_attempts'].double()
                mean, slow, pct = idle(att)
                say('%s %s %8.3f / %8.3f / %8.3f ms   attempts %4d / %6.1f / %4d (rows)   per wavefront: mean %.1f, slowest lane %.1f, lanes idle %.0f %%'
                    % ((head, name) + res + (int(att.min()), float(att.mean()), int(att.max()), mean, slow, pct)))
                if name.startswith('(b)'):
                    # where (b) - (a) goes: the same call with the per-row inputs validated ONCE, outside the timed region (what is left is
                    # the solver object, the launch and the status read, as in (a))
                    from tfdiffeq_amd import rows_times
                    from tfdiffeq_amd.misc import _check_inputs
                    from tfdiffeq_amd.odeint import SOLVERS
                    rt, o2 = rows_times.prepare(y0, t, tol['rtol'], tol['atol'], on)

                    def launch_only():
                        _, f2, state, _ = _check_inputs(f, y0, [0., 1.])
                        return SOLVERS['dopri5'](f2, state, rtol=rt.rtol0, atol=rt.atol0, **o2).integrate_rows_t(rt)
                    res = timed(launch_only, args.steps, args.warmup)
                    say('%s (b) without the validation of t %8.3f / %8.3f / %8.3f ms' % ((head,) + res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
