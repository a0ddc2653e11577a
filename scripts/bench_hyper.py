"""Hypersolver benchmark (JSON lines; bench.py is not involved).

  notebook   the reference notebook's predict(): HyperHeun, batch 1, 10 000 points, float64, g 7-64-64-64-3 PReLU - the fused engine
             against the eager torch loop on the GPU, beside the notebook's published CPU time (7.73 s)
  batched    65 536 Lorenz trajectories x 1 001 points, HyperEuler / HyperHeun, float32 / float64: state elements per second and g's
             FLOPs over the call's wall time as a fraction of the matrix-core peak of the dtype

Times are medians of timed calls after warm-up calls, each bracketed by torch.cuda.synchronize(): whole calls (Python, the launch and
the kernel), not kernel times.
    python scripts/bench_hyper.py [--repeats 5]
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
PUBLISHED_PREDICT_S = 7.73                                     # examples/hyper_solvers.ipynb of the reference, CPU


def notebook_g(dtype, dev):
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64),
                         nn.Linear(64, 3)).to(device=dev, dtype=dtype).requires_grad_(False)


def g_flops(g):
    return sum(2 * m.in_features * m.out_features for m in g if isinstance(m, nn.Linear))


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
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lor = rhs.Lorenz()

    # notebook predict: batch 1, 10 000 points
    g = notebook_g(torch.float64, dev)
    s = hyper_solvers.HyperHeun(lor, g)
    t = torch.arange(0, 100, 0.01, dtype=torch.float64, device=dev)
    y0 = torch.tensor([[1., 1., 1.]], dtype=torch.float64, device=dev)
    with torch.no_grad():
        fused_s, fused_all = median_time(lambda: s.trajectory(t, y0), 2, args.repeats)
        assert s.last_stats['engine'] == 'fused'
        launches = s.last_stats['n_launches']
        ref = s.trajectory(t, y0)
        eager_s, eager_all = median_time(lambda: s._eager(0, t, y0), 1, 3)
        eager = s._eager(0, t, y0)
    print(json.dumps({'workload': 'notebook_predict', 'method': 'HyperHeun', 'batch': 1, 'points': int(t.shape[0]), 'dtype': 'float64',
                      'g': s.last_stats['g'] if s.last_stats.get('g') else '7-64-64-64-3 PReLU', 'fused_s': fused_s, 'fused_runs_s': fused_all,
                      'fused_launches': launches, 'eager_gpu_s': eager_s, 'eager_runs_s': eager_all, 'published_cpu_s': PUBLISHED_PREDICT_S,
                      'speedup_vs_eager': eager_s / fused_s, 'speedup_vs_published': PUBLISHED_PREDICT_S / fused_s,
                      'max_abs_diff_fused_eager': float((ref - eager).abs().max())}), flush=True)

    # batched: 65 536 x 1 001
    B, T = 65536, 1001
    for dtype in (torch.float32, torch.float64):
        g = notebook_g(dtype, dev)
        t = torch.linspace(0., 10., T, dtype=dtype, device=dev)
        gen = torch.Generator().manual_seed(1)
        y0 = (torch.ones(B, 3, dtype=torch.float64) + 0.1 * torch.randn(B, 3, generator=gen, dtype=torch.float64)).to(device=dev, dtype=dtype)
        for cls, evals in ((hyper_solvers.HyperEuler, 1), (hyper_solvers.HyperHeun, 2)):
            s = cls(lor, g)
            with torch.no_grad():
                sec, runs = median_time(lambda: s.trajectory(t, y0), 1, args.repeats)
                out = s.trajectory(t, y0)
            assert s.last_stats['engine'] == 'fused'
            flop = float(g_flops(g)) * evals * B * (T - 1)
            print(json.dumps({'workload': 'batched', 'method': cls.__name__, 'batch': B, 'points': T, 'dtype': str(dtype).replace('torch.', ''),
                              'call_s': sec, 'runs_s': runs, 'launches': s.last_stats['n_launches'],
                              'state_elements_per_s': B * (T - 1) * 3 / sec, 'g_flop': flop, 'g_tflops': flop / sec / 1e12,
                              'g_fraction_of_mfma_peak': flop / sec / 1e12 / PEAK_TFLOPS[dtype], 'peak_tflops': PEAK_TFLOPS[dtype],
                              'finite': bool(torch.isfinite(out).all())}), flush=True)
            del out


if __name__ == '__main__':
    main()
