"""Shared against per-trajectory step control on the same inputs (options={'per_trajectory': True}, csrc/mi_ode_rows.h).

Shape: config 3 of bench.py - 65 536 Lorenz systems, t = [0, 1], rtol 1e-6, atol 1e-9 - with two sets of initial conditions:
  bench    bench.py's own (seed 1: [1, 1, 1] + 1e-3 randn): every row needs about the same steps;
  spread   the 70 spread rows of the tests (tests/per_trajectory_cases.py `base_y0`: 3.3 decades) tiled to the batch.
dopri5 and tsit5, float64 and float32 (float32: rtol 1e-4, atol 1e-6).  For both modes: ms per call (in-run HIP events, min / median / max of
the timed calls after the warm-up), attempts (shared: the call's count; per-trajectory: min / mean / max over the rows) and state elements per
second (batch x 3 / median).  Same tree, same process, same inputs.

usage: python scripts/bench_per_trajectory.py [--steps 20] [--warmup 5] [--batch 65536] [--out profiles/per_trajectory_bench.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import per_trajectory_cases as PC  # noqa: E402
from tfdiffeq_amd import odeint, rhs  # noqa: E402


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'per_trajectory_bench.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = ['# scripts/bench_per_trajectory.py --steps %d --warmup %d --batch %d: %s; Lorenz, t = [0, 1]; ms per call min / median / max'
             % (args.steps, args.warmup, args.batch, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    inputs = {'bench ': torch.tensor(np.array([1., 1., 1.]) + 1e-3 * rng.standard_normal((args.batch, 3))),
              'spread': PC.base_y0().repeat(-(-args.batch // 70), 1)[:args.batch].contiguous()}
    t = torch.tensor([0., 1.], dtype=torch.float64)
    f = rhs.Lorenz()
    for label, y64 in inputs.items():
        for dtype, tol in ((torch.float64, dict(rtol=1e-6, atol=1e-9)), (torch.float32, dict(rtol=1e-4, atol=1e-6))):
            y0 = y64.to(device=dev, dtype=dtype)
            for method in ('dopri5', 'tsit5'):
                head = 'y0 %s %-7s %-6s' % (label, str(dtype).replace('torch.', ''), method)
                res = timed(lambda: odeint(f, y0, t, method=method, **tol), args.steps, args.warmup)
                st = dict(odeint.last_stats)
                assert st.get('per_trajectory') is None and st['n_launches'] == 1, st
                say('%s  shared          %8.3f / %8.3f / %8.3f ms   attempts %4d                      %8.2f M elements/s'
                    % ((head,) + res + (st['n_attempts'], args.batch * 3 / res[1] / 1e3)))
                res = timed(lambda: odeint(f, y0, t, method=method, options={'per_trajectory': True}, **tol), args.steps, args.warmup)
                st = dict(odeint.last_stats)
                assert st['per_trajectory'] is True and st['n_launches'] == 1, st
                att = st['rows']['n_attempts'].double()
                say('%s  per-trajectory  %8.3f / %8.3f / %8.3f ms   attempts %4d / %6.1f / %4d (rows)  %8.2f M elements/s'
                    % ((head,) + res + (int(att.min()), float(att.mean()), int(att.max()), args.batch * 3 / res[1] / 1e3)))
                # where a wavefront's time goes: it runs until its slowest lane ends
                per_wave = att[:att.numel() // 64 * 64].reshape(-1, 64)
                say('%s                  attempts per wavefront: mean of the 64 lanes %.1f, slowest lane %.1f (lanes idle %.0f %% of the loop)'
                    % (head, float(per_wave.mean()), float(per_wave.max(dim=1).values.mean()),
                       100.0 * (1.0 - float(per_wave.mean()) / float(per_wave.max(dim=1).values.mean()))))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
