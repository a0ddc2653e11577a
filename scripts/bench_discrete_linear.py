"""A full training step (forward + loss + backward) of models.LinearODEFunc with the gradient of the discrete map, three ways, in float64 at
65536 x 128 (config 4's shape) and 4096 x 128 and in float32 at 65536 x 64, for rk4 on 5 and 21 grid points and one-step Euler:

  taped    the solver loop written in torch ops and back-propagated - what a user has to write without odeint_discrete
           (tests/discrete_restatement.py);
  generic  ODEBlock(gradient='discrete') with the generic sweep (discrete.LINEAR = False): fused forward, one taped step + one
           torch.autograd.grad call per grid interval backward;
  fused    the same block with discrete.LINEAR = 'auto': fused forward, the whole backward in one launch (csrc/mi_ode_discrete_linear.h).

One process, in-run HIP events, min / median / max over the timed steps after the warm-up.  The kernel alone comes from the engine's own
profile record (workgroup 0's clock: tile sweep with the weight-gradient products, partial-block store, final hand-off + fold), median over
the same number of blocking sweep calls; its fraction of the matrix peak (78.6 TFLOP/s float64, 157.3 float32) follows from
2 dim^2 rows (S - 1 + 2 S) flops per step: S - 1 forward evaluations, S transposed ones, S weight-gradient products.

usage: python scripts/bench_discrete_linear.py [--steps 20] [--warmup 5] [--out profiles/discrete_linear_bench.txt] [--only fused]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tfdiffeq_amd import discrete, models, odeint_discrete  # noqa: E402
from tests import discrete_restatement as DR  # noqa: E402

PEAK = {torch.float64: 78.6e12, torch.float32: 157.3e12}
SHAPES = ((65536, 128, torch.float64), (4096, 128, torch.float64), (65536, 64, torch.float32))


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'discrete_linear_bench.txt'))
    ap.add_argument('--only', default='', help='comma-separated subset of taped,generic,fused')
    args = ap.parse_args()
    only = set(filter(None, args.only.split(',')))
    dev = torch.device('cuda:0')
    lines = ['# scripts/bench_discrete_linear.py --steps %d --warmup %d: %s, models.LinearODEFunc with bias; ms per training step (min / median / max)'
             % (args.steps, args.warmup, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for batch, dim, dtype in SHAPES:
        torch.manual_seed(0)
        func = models.LinearODEFunc(dim, bias=True, dtype=dtype).to(dev)
        x = torch.randn(batch, dim, device=dev, dtype=dtype)
        w = torch.randn(batch, dim, device=dev, dtype=dtype)
        for method, n in (('rk4', 5), ('rk4', 21), ('euler', 2)):
            t = torch.linspace(0., 1., n, dtype=dtype)
            block = models.ODEBlock(func, solver=method, gradient='discrete')

            def zero():
                for p in func.parameters():
                    p.grad = None

            def taped():
                zero()
                xi = x.clone().requires_grad_(True)
                (DR.solve(func, xi, t, method)[-1] * w).sum().backward()

            def block_step():
                zero()
                xi = x.clone().requires_grad_(True)
                (block(xi, eval_times=t)[-1] * w).sum().backward()

            head = '%5d x %3d %s %-5s N=%2d' % (batch, dim, str(dtype).replace('torch.', ''), method, n)
            if not only or 'taped' in only:
                say('%s  taped torch loop      %9.3f / %9.3f / %9.3f' % ((head,) + timed(taped, args.steps, args.warmup)))
            if not only or 'generic' in only:
                discrete.LINEAR = False
                res = timed(block_step, args.steps, args.warmup)
                assert odeint_discrete.last_backward_stats['engine'] == 'generic sweep'
                say('%s  generic sweep         %9.3f / %9.3f / %9.3f' % ((head,) + res))
            if only and 'fused' not in only:
                continue
            discrete.LINEAR = 'auto'
            res = timed(block_step, args.steps, args.warmup)
            st = odeint_discrete.last_backward_stats
            assert st['engine'] == 'fused linear sweep' and st['n_launches'] == 1, st
            discrete.LINEAR = False
            # the kernel alone: the engine's blocking sweep call on the last forward solution, timed by the kernel's own record
            eng = discrete._cached_linear_engine(batch, dim, True, method, n, str(dev), dtype)
            with torch.no_grad():
                ys = block(x, eval_times=t).contiguous()
            gys = torch.zeros_like(ys)
            gys[-1] = w
            tt = t.double().numpy()
            W, b = func.weight.detach(), func.bias.detach()
            recs = []
            for i in range(args.warmup + args.steps):
                eng.sweep(W, b, tt, ys, gys)
                if i >= args.warmup:
                    recs.append(eng.profile())
            sweep, store, fold = (statistics.median(r[k] for r in recs) for k in ('sweep_us', 'store_us', 'fold_us'))
            total = statistics.median(r['sweep_us'] + r['store_us'] + r['fold_us'] for r in recs)
            S = DR.STAGES[method]
            flops = 2.0 * dim * dim * batch * (S - 1 + 2 * S) * (n - 1)
            say('%s  fused linear sweep    %9.3f / %9.3f / %9.3f   kernel alone %8.3f ms (grid %d: tile sweep %.1f us, partial store %.1f us, hand-off + fold %.1f us)'
                ' = %.1f %% of the %s matrix peak'
                % ((head,) + res + (total * 1e-3, recs[-1]['grid'], sweep, store, fold, 100.0 * flops / (total * 1e-6) / PEAK[dtype],
                                     'float64' if dtype == torch.float64 else 'float32')))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
