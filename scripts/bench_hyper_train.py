"""Hypersolver training benchmark (JSON lines; bench.py is not involved): ONE optimizer step - forward, backward, Adam - of HyperHeun on
Lorenz with the notebook's g (7-64-64-64-3 PReLU), the fused gradient (options={'grad': 'auto'}, csrc/mi_ode_hyper_grad.h) against the
eager engine (the option unset: the default path), at three shapes:

  notebook     the reference notebook's cells 15 / 17: float64, batch 1, T = 16
  pretraining  examples/hyper_solvers.py's simplified pretraining: float64, batch 16, T = 2, the loss on the last row
  large        float32, batch 4096, T = 17

Per shape: medians of whole optimizer steps after warm-up, host clock around a device synchronise; the backward launch alone from HIP
events; g's forward + backward FLOPs over the fused step as a fraction of the dtype's matrix-core peak (the gradient kernel evaluates g
three times per Heun step and applies two transposed products per layer and evaluation).
    python scripts/bench_hyper_train.py [--repeats 20] [--only fused|eager]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import hyper_solvers, rhs  # noqa: E402

PEAK_TFLOPS = {torch.float64: 78.6, torch.float32: 157.3}     # MI355X matrix cores, dense
SHAPES = [('notebook', torch.float64, 1, 16, False), ('pretraining', torch.float64, 16, 2, True), ('large', torch.float32, 4096, 17, False)]


def notebook_g(dtype, dev):
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64),
                         nn.Linear(64, 3)).to(device=dev, dtype=dtype)


def median_time(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=['fused', 'eager'], default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name, dtype, B, T, last_only in SHAPES:
        t = torch.arange(T, dtype=dtype, device=dev) * 0.01
        gen = torch.Generator().manual_seed(1)
        y0 = (torch.ones(B, 3, dtype=torch.float64) + 0.1 * torch.randn(B, 3, generator=gen, dtype=torch.float64)).to(device=dev, dtype=dtype)
        target = torch.randn(T, B, 3, generator=gen, dtype=torch.float64).to(device=dev, dtype=dtype)
        row = {'workload': name, 'method': 'HyperHeun', 'dtype': str(dtype).replace('torch.', ''), 'batch': B, 'T': T, 'loss_on_last_row': last_only}
        for engine, opt_grad in (('fused', 'auto'), ('eager', False)):
            if args.only not in (None, engine):
                continue
            g = notebook_g(dtype, dev)
            s = hyper_solvers.HyperHeun(rhs.Lorenz(), g, options={'grad': opt_grad})
            opt = torch.optim.Adam(g.parameters(), lr=1e-4)

            def step():
                out = s.trajectory(t, y0)
                loss = (out[-1] - target[-1]).pow(2).mean() if last_only else (out - target).pow(2).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
            sec, runs = median_time(step, 3, args.repeats if engine == 'fused' or B < 1024 else max(3, args.repeats // 4))
            assert s.last_stats['engine'] == engine, s.last_stats
            row[engine + '_step_s'] = sec
            row[engine + '_step_min_max_s'] = [min(runs), max(runs)]
            if engine == 'fused':
                row['backward_stats'] = dict(s.last_backward_stats)
                out = s.trajectory(t, y0)
                G = torch.ones_like(out)
                evs = []
                for _ in range(5):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    out = s.trajectory(t, y0)
                    a.record()
                    out.backward(G)
                    b.record()
                    torch.cuda.synchronize()
                    evs.append(a.elapsed_time(b) * 1e-3)
                row['backward_events_s'] = statistics.median(evs)      # the gradient launch(es) with autograd's dispatch around them
                macs = sum(m.in_features * m.out_features for m in g if isinstance(m, nn.Linear))
                flop = 2.0 * macs * B * (T - 1) * (2 + 3 + 2 * 2 * 2)  # forward: 2 evaluations; backward: 3 evaluations + 2 x (delta W, X^T delta)
                row['g_flop'] = flop
                row['g_fraction_of_mfma_peak'] = flop / sec / 1e12 / PEAK_TFLOPS[dtype]
        if 'fused_step_s' in row and 'eager_step_s' in row:
            row['speedup'] = row['eager_step_s'] / row['fused_step_s']
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
