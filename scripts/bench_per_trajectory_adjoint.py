"""One training step (forward + backward) of a Lorenz ensemble: the per-trajectory adjoint against the only route the tree had before it.

Shape: 65 536 Lorenz systems (tests/per_trajectory_adjoint_cases.LorenzModule: sigma, rho, beta trainable), t = [0, 1], dopri5, float64 at
rtol 1e-6 / atol 1e-9 and float32 at 1e-4 / 1e-6, two sets of initial conditions (as scripts/bench_per_trajectory.py):
  bench    bench.py's own (seed 1: [1, 1, 1] + 1e-3 randn): every row needs about the same steps;
  spread   the 70 spread rows of the tests (3.3 decades) tiled to the batch.
Two routes, same tree, same process, same inputs, loss = sum(solution[-1] ** 2):
  per-trajectory   odeint_adjoint(..., options={'per_trajectory': True}): forward k_rows_rowlocal, backward k_rows_adjoint, one launch each;
  shared           odeint_adjoint(...) without the option: shared control over the augmented state of the WHOLE batch, the plane kernels,
                   one torch.autograd.grad per stage.
The two compute different things by design (every row its own solve / one solve of the batch); the table is what a user pays for a
training step either way.  ms per step: in-run HIP events, min / median / max of the timed steps after the warm-up.

usage: python scripts/bench_per_trajectory_adjoint.py [--steps 20] [--warmup 5] [--batch 65536] [--out profiles/per_trajectory_adjoint_bench.txt]
"""
import argparse
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import per_trajectory_adjoint_cases as AC  # noqa: E402
import per_trajectory_cases as PC  # noqa: E402
from tfdiffeq_amd import odeint_adjoint  # noqa: E402


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'per_trajectory_adjoint_bench.txt'))
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    dev = torch.device('cuda:0')
    lines = ['# scripts/bench_per_trajectory_adjoint.py --steps %d --warmup %d --batch %d: %s; Lorenz module (3 trainable scalars), t = [0, 1], dopri5; '
             'one training step (forward + backward), ms min / median / max' % (args.steps, args.warmup, args.batch, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    inputs = {'bench ': torch.tensor(np.array([1., 1., 1.]) + 1e-3 * rng.standard_normal((args.batch, 3))),
              'spread': PC.base_y0().repeat(-(-args.batch // 70), 1)[:args.batch].contiguous()}
    t = torch.tensor([0., 1.], dtype=torch.float64)
    for label, y64 in inputs.items():
        for dtype, tol in ((torch.float64, dict(rtol=1e-6, atol=1e-9)), (torch.float32, dict(rtol=1e-4, atol=1e-6))):
            mod = AC.LorenzModule(dtype, dev)
            y0 = y64.to(device=dev, dtype=dtype).requires_grad_(True)
            head = 'y0 %s %-7s' % (label, str(dtype).replace('torch.', ''))

            def step(options):
                for p in mod.parameters():
                    p.grad = None
                y0.grad = None
                sol = odeint_adjoint(mod, y0, t, method='dopri5', options=options, **tol)
                sol[-1].pow(2).sum().backward()

            res = timed(lambda: step({'per_trajectory': True}), args.steps, args.warmup)
            st = dict(odeint_adjoint.last_backward_stats)
            assert st['per_trajectory'] is True and st['n_launches'] == 1 and st['forward']['n_launches'] == 1, st
            att = st['rows']['n_attempts'].sum(dim=1).double()
            say('%s  per-trajectory  %9.3f / %9.3f / %9.3f ms   backward attempts per row %4d / %6.1f / %4d   %8.2f M state elements/s'
                % ((head,) + res + (int(att.min()), float(att.mean()), int(att.max()), args.batch * 3 / res[1] / 1e3)))
            per_wave = att[:att.numel() // 64 * 64].reshape(-1, 64)
            say('%s                  backward attempts per wavefront: mean of the 64 lanes %.1f, slowest lane %.1f (lanes idle %.0f %% of the loop)'
                % (head, float(per_wave.mean()), float(per_wave.max(dim=1).values.mean()),
                   100.0 * (1.0 - float(per_wave.mean()) / float(per_wave.max(dim=1).values.mean()))))
            res = timed(lambda: step(None), args.steps, args.warmup)
            st = dict(odeint_adjoint.last_backward_stats)
            assert st.get('per_trajectory') is None, st
            say('%s  shared          %9.3f / %9.3f / %9.3f ms   backward engine: %s   %8.2f M state elements/s'
                % ((head,) + res + (st.get('engine'), args.batch * 3 / res[1] / 1e3)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
