"""Conv2dODEFunc benchmark (JSON lines; bench.py is not involved): the fused stage kernel (rhs.Conv2dODE, csrc/mi_ode_conv.h) against
the same module's torch forward on the callable engine (graph 'auto'), per shape:

  call_ms_fused / call_ms_torch   one odeint(dopri5, t = [0, 1], rtol = atol = 1e-3) call, inference, float32: medians of timed calls
                                  after warm-up calls, each bracketed by torch.cuda.synchronize() (Python, launches and kernels)
  stage_us                        one fused evaluation (k_conv_stage, no stage combination): median over repeats of a batch of 20
                                  back-to-back launches timed with events
  conv2_frac_of_peak              conv2's FLOPs (2 B H W 9 F^2) over stage_us, as a fraction of the float32 matrix peak (157.3 TF)

Then a batch sweep at the MNIST shape with 5 augment channels (6 x 28 x 28, F = 64), B = 1 .. 256: where the fused path stops being
the faster route (rhs.Conv2dODE.FUSED_MAX_CONV2_FLOP is placed from it).  Every line records the engine string of the fused call.

    python scripts/bench_conv.py [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import models, odeint  # noqa: E402

PEAK_TFLOPS = {torch.float64: 78.6, torch.float32: 157.3}     # MI355X matrix cores, dense
SHAPES = [('reference test', 10, 3, 0, 5, 5, 10), ('mnist', 256, 1, 0, 28, 28, 92), ('mnist aug5', 256, 1, 5, 28, 28, 64),
          ('cifar', 128, 3, 0, 32, 32, 125), ('cifar aug10', 128, 3, 10, 32, 32, 64)]


def median_call(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--dtype', default='float32', choices=['float32', 'float64'])
    args = ap.parse_args()
    dtype = getattr(torch, args.dtype)
    dev = torch.device('cuda:0')
    warnings.simplefilter('ignore')
    for name, B, C, aug, H, W, F in SHAPES:
        measure(name, B, C, aug, H, W, F, dtype, dev, args.repeats)
    for B in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        measure('sweep mnist aug5', B, 1, 5, 28, 28, 64, dtype, dev, args.repeats)


def measure(name, B, C, aug, H, W, F, dtype, dev, repeats):
    torch.manual_seed(0)
    fn = models.Conv2dODEFunc(C, F, augment_dim=aug).to(dev, dtype)
    desc = fn.device_rhs()
    y0 = 0.5 * torch.randn(B, C + aug, H, W, device=dev, dtype=dtype)
    t = torch.tensor([0., 1.], dtype=torch.float64)
    res = {}
    with torch.no_grad():
        for key, f in (('fused', desc), ('torch', fn)):
            res['call_ms_' + key] = 1e3 * median_call(lambda: odeint(f, y0, t, rtol=1e-3, atol=1e-3), 2, repeats)
            res['nfe_' + key] = int(odeint.last_stats.get('nfe', 0))
            res['engine_' + key] = odeint.last_stats.get('engine')
        tt = torch.zeros((), dtype=dtype, device=dev)
        for _ in range(3):
            desc.stage(tt, y0)
        per = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                desc.stage(tt, y0)
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / 20)
        stage_us = statistics.median(per)
    flops = 2.0 * B * H * W * 9 * F * F
    print(json.dumps(dict(shape=name, batch=B, channels=C + aug, hw=[H, W], filters=F, dtype=str(dtype).replace('torch.', ''),
                          stage_us=round(stage_us, 2), conv2_gflop=round(flops / 1e9, 4),
                          conv2_frac_of_peak=round(flops / (stage_us * 1e-6) / (PEAK_TFLOPS[dtype] * 1e12), 4),
                          speedup=round(res['call_ms_torch'] / res['call_ms_fused'], 2),
                          **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()})), flush=True)

if __name__ == '__main__':
    main()
