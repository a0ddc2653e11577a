"""GPU test of bench.py's two kinds of run.  A plain run (`--gpus 1 --steps N --warmup W`) does what its headline figure needs and no more;
`--full` adds, after the timed steps, what takes runs of its own (the CPU baseline with the parity check, the sustained loop with the board's
telemetry, the per-stage schedule's roofline).  Each run is a new process, as the benchmark is run, and its wall time is taken from outside.

The bound on the plain run is the one the project sets for it: at most 30 s of the whole run, start to exit, outside its N + W steps
(wall - (N + W) x ms_per_step), loading the kernels at the first step included."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTSIDE_STEPS_MAX_S = 30.0
CONTRACT = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data',
            'config', 'roofline', 'cpu_baseline')


def _bench(*argv, timeout=600):
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().split('\n')
    assert len(lines) == 1, lines                           # ONE line on stdout
    return json.loads(lines[0]), wall


def _check_headline(d, steps, warmup):
    for k in CONTRACT:
        assert k in d, k
    assert d['metric'] == 'state-elements/sec (batch x dim / wall-s) Dopri5 float64' and d['unit'] == 'state-elements/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'f64' and d['n_gpus'] == 1 and d['steps'] == steps and d['warmup'] == warmup
    assert abs(d['value'] - 65536 * 128 / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
    r = d['roofline']
    assert r['bound'] == 'mfma' and 0 < r['avg_launch_ms'] <= d['ms_per_step'] and r['launches_timed'] == steps
    assert d['config']['kernel_launches'] == 1 and d['config']['attempts_per_step'] > 0


def test_plain_run_is_lean(tmp_path):
    steps, warmup = 10, 2
    d, wall = _bench('--gpus', '1', '--steps', str(steps), '--warmup', str(warmup), '--dump-outputs', str(tmp_path / 'dump'))
    outside = wall - (steps + warmup) * d['ms_per_step'] * 1e-3
    print('plain run: wall %.2f s, ms_per_step %.4f, outside its steps %.2f s' % (wall, d['ms_per_step'], outside))
    _check_headline(d, steps, warmup)
    assert d['full'] is False
    # what takes runs of its own is not there ...
    assert d['cpu_baseline'] is None and 'parity_max_abs_diff' not in d and 'parity_attempts' not in d
    assert 'roofline_per_stage_schedule' not in d and 'transport_survey' not in d['config']
    smi = d['config']['smi']
    assert 'sustained_loop' not in smi and 'before_warmup' in smi and 'after_timed_steps' in smi
    # ... the dump is
    import numpy as np
    sol = np.load(str(tmp_path / 'dump' / 'solution.npy'))
    assert list(sol.shape) == d['dumped_outputs']['shape'] and sol.dtype == np.float64 and np.isfinite(sol).all()
    assert outside <= OUTSIDE_STEPS_MAX_S, outside


def test_full_run_adds_the_other_measurements():
    """--full with --no-cpu-baseline: everything --full adds but the 50 s CPU leg, which has its own switch."""
    steps, warmup = 3, 1
    d, _ = _bench('--gpus', '1', '--steps', str(steps), '--warmup', str(warmup), '--full', '--no-cpu-baseline')
    _check_headline(d, steps, warmup)
    assert d['full'] is True and d['cpu_baseline'] is None
    s = d['roofline_per_stage_schedule']
    assert s['bound'] == 'hbm' and s['launches_timed'] >= 5 and s['avg_launch_ms'] > 0 and s['ms_per_step_with_this_schedule'] > 0
    smi = d['config']['smi']
    if smi['before_warmup']:                                 # (a host that exposes the board's hwmon files)
        loop = smi['sustained_loop']
        assert loop['calls'] > 0 and loop['seconds'] >= 1.5 and loop['kernel_clock_mhz'] > 0
