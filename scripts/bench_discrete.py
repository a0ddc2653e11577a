"""A full training step (forward + loss + backward) with the gradient of the discrete map, three ways, at config 5's shape (64-128-128-64
tanh, float32, batch 32768) and at batch 4096, for rk4 on 5 and 21 grid points and one-step Euler:

  taped    the solver loop written in torch ops and back-propagated - what a user has to write without odeint_discrete
           (tests/discrete_restatement.py);
  generic  ODEBlock(gradient='discrete') with the generic sweep (discrete.FUSED = False): fused forward, one taped step + one
           torch.autograd.grad call per grid interval backward;
  fused    ODEBlock(gradient='discrete'): fused forward, the whole backward in one launch (csrc/mi_ode_discrete.h).

One process, in-run HIP events, min / median / max over the timed steps after the warm-up.  The fused kernel alone is timed too; its
fraction of the fp32 matrix peak (157.3 TFLOP/s) follows from its own multiply-add count: forward recompute, backward data and weight
gradients, 3 x (d h + h h + h d) per row, stage and step.

--time-dependent: ODEFunc(time_dependent=True) - the first layer sees concat([t, x]); the fused kernel then adds the stage time's bias
shift and the gradient of w_t (the multiply-add count above is unchanged: w_t is one more bias-like sum).

--float64: the same table for the float64 network with discrete.MLP64 = 'auto' (csrc/mi_ode_discrete64.h; without the switch a float64
network takes the generic sweep, which is the `generic` row); the kernel-alone column is then a fraction of the fp64 matrix peak
(78.6 TFLOP/s) and is followed by the kernel's own profile triple (workgroup 0: tile passes, weight-gradient passes, hand-off + fold).
Combinable with --time-dependent.

usage: python scripts/bench_discrete.py [--steps 20] [--warmup 5] [--chunks 0,1] [--out FILE] [--only fused] [--time-dependent] [--float64]
(--out defaults to profiles/discrete_bench.txt, to profiles/discrete_td_bench.txt with --time-dependent, to profiles/discrete_f64_bench.txt
with --float64 and to profiles/discrete_f64_td_bench.txt with both)
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

PEAK = 157.3e12
PEAK64 = 78.6e12
DIM, HID = 64, 128


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
    ap.add_argument('--chunks', default='0,1', help='tiles per weight-gradient pass of the fused kernel to compare (0: all of a workgroup\'s)')
    ap.add_argument('--out', default='', help='default: profiles/discrete_bench.txt, profiles/discrete_td_bench.txt with --time-dependent')
    ap.add_argument('--only', default='', help='comma-separated subset of taped,generic,fused')
    ap.add_argument('--time-dependent', action='store_true', help='the time-dependent network (fc1 sees concat([t, x]))')
    ap.add_argument('--float64', action='store_true', help="the float64 network on the opt-in float64 sweep (discrete.MLP64 = 'auto')")
    args = ap.parse_args()
    if args.float64:
        default_out = 'discrete_f64_td_bench.txt' if args.time_dependent else 'discrete_f64_bench.txt'
    else:
        default_out = 'discrete_td_bench.txt' if args.time_dependent else 'discrete_bench.txt'
    args.out = args.out or os.path.join(ROOT, 'profiles', default_out)
    dtype = torch.float64 if args.float64 else torch.float32
    name = 'fused mlp sweep (float64)' if args.float64 else 'fused mlp sweep'
    peak, peak_name = (PEAK64, 'fp64') if args.float64 else (PEAK, 'fp32')
    if args.float64:
        discrete.MLP64 = 'auto'
    only = set(filter(None, args.only.split(',')))
    dev = torch.device('cuda:0')
    lines = ['# scripts/bench_discrete.py --steps %d --warmup %d%s%s: %s, 64-128-128-64 tanh %s%s; ms per training step (min / median / max)'
             % (args.steps, args.warmup, ' --float64' if args.float64 else '', ' --time-dependent' if args.time_dependent else '',
                torch.cuda.get_device_name(0), 'float64' if args.float64 else 'float32', ', time dependent' if args.time_dependent else '')]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for batch in (32768, 4096):
        torch.manual_seed(0)
        func = models.ODEFunc(DIM, HID, time_dependent=args.time_dependent, non_linearity='tanh').to(dev).to(dtype)
        x = torch.randn(batch, DIM, device=dev, dtype=dtype)
        w = torch.randn(batch, DIM, device=dev, dtype=dtype)
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

            head = 'batch %5d %-5s N=%2d' % (batch, method, n)
            if not only or 'taped' in only:
                say('%s  taped torch loop      %9.3f / %9.3f / %9.3f' % ((head,) + timed(taped, args.steps, args.warmup)))
            if not only or 'generic' in only:
                discrete.FUSED = False
                res = timed(block_step, args.steps, args.warmup)
                assert odeint_discrete.last_backward_stats['engine'] == 'generic sweep'
                say('%s  generic sweep         %9.3f / %9.3f / %9.3f' % ((head,) + res))
            if only and 'fused' not in only:
                continue
            discrete.FUSED = True
            for chunk in [int(c) for c in args.chunks.split(',')]:
                discrete.CHUNK_TILES = chunk
                res = timed(block_step, args.steps, args.warmup)
                st = odeint_discrete.last_backward_stats
                assert st['engine'] == name and st['n_launches'] == 1, st
                # the kernel alone: the engine's blocking sweep call on the last forward solution
                cached = discrete._cached_engine64 if args.float64 else discrete._cached_engine
                eng = cached(batch, DIM, HID, method, n, str(dev), chunk, args.time_dependent)
                with torch.no_grad():
                    ys = block(x, eval_times=t).contiguous()
                gys = torch.zeros_like(ys)
                gys[-1] = w
                tt = t.double().numpy()
                mlp = func.device_rhs()
                k = timed(lambda: eng.sweep(mlp, tt, ys, gys), args.steps, args.warmup)
                mac = batch * (n - 1) * DR.STAGES[method] * 3 * (DIM * HID + HID * HID + HID * DIM)
                prof = '   profile us: tile passes %.0f, weight-gradient passes %.0f, hand-off + fold %.0f' % eng.profile() if args.float64 else ''
                say('%s  fused sweep chunk=%-3d %9.3f / %9.3f / %9.3f   kernel alone %8.3f / %8.3f / %8.3f ms = %.1f %% of the %s matrix peak (median)%s'
                    % ((head, chunk) + res + k + (100.0 * 2 * mac / (k[1] * 1e-3) / peak, peak_name, prof)))
            discrete.CHUNK_TILES = 0
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
