#!/usr/bin/env python3
"""Per-row IIR stage (distortion.IirStage with one cascade per row, kernel iir_rows_tile) against the two things
the tree could do before it, timed with device events in ONE process per shape:

    python tools/iir_rows_bench.py [--shapes awg,256x1e7,8x1e7] [--reps 20] [--json out.json]

  (a) loop    one prebuilt IirPlan(batch=1) per row, launched in a Python loop (plan building outside the timed
              region) -- the only way to give every row its own filter without the per-row plan; shape `awg` only
  (b) rows    IirRowsPlan, one launch, a distinct three-time-constant correction per row (one section of order 3)
  (c) shared  IirPlan(batch=rows) with ONE cascade for all rows on the same bytes: not the same job, a yardstick
              of what the shape allows
ms = median of --reps after a warm-up; GB/s on 16 B/sample (x read once, y written once).  Every shape runs in a
child process of its own under a time limit; the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {'awg': (2048, 10**5), '256x1e7': (256, 10**7), '8x1e7': (8, 10**7)}
RATE = 2e9


def timed(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def row_filters(rows, seed=0):
    """one combined (b, a) of three exp-decay corrections per row, all different"""
    from waveforms_amd import distortion
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rows):
        taus = [rng.uniform(20e-9, 40e-9), rng.uniform(80e-9, 200e-9), rng.uniform(0.5e-6, 5e-6)]
        amps = rng.uniform(0.005, 0.03, 3) * rng.choice([-1, 1], 3)
        out.append(distortion.combine_filters([distortion.exp_decay_filter(A, t, RATE) for A, t in zip(amps, taus)]))
    return out


def run_shape(name, reps, only=None):
    import torch
    from scipy.signal import lfilter
    from waveforms_amd import _engine, distortion
    rows, n = SHAPES[name]
    dev = torch.device('cuda', 0)
    x = torch.randn(rows, n, dtype=torch.float64, device=dev)
    y = torch.empty_like(x)
    filt = row_filters(rows)
    stream = torch.cuda.current_stream(dev).cuda_stream
    r = dict(shape=name, rows=rows, n=n, dtype='float64', bytes_per_sample=16)
    gbs = lambda ms: round(rows * n * 16 / ms / 1e6, 1)
    if only in (None, 'rows'):
        st = distortion.IirStage([[f] for f in filt], n, rows)
        r['rows_kernel'] = st.kernel_name()
        r['rows_ms'] = round(timed(lambda: st.apply_torch(x, out=y), reps), 4)
        r['rows_gbs'] = gbs(r['rows_ms'])
        probe = [0, rows // 2, rows - 1]
        m = min(n, 200000)
        got = y[probe, :m].cpu().numpy()
        xs = x[probe, :m].cpu().numpy()
        r['rows_max_err_vs_lfilter'] = float('%.3g' % max(np.max(np.abs(got[i] - lfilter(*filt[p], xs[i])))
                                                          for i, p in enumerate(probe)))
        st.close()
    if only in (None, 'shared'):
        sh = distortion.IirStage([filt[0]], n, rows)
        r['shared_ms'] = round(timed(lambda: sh.apply_torch(x, out=y), reps), 4)
        r['shared_gbs'] = gbs(r['shared_ms'])
        sh.close()
    if name == 'awg' and only in (None, 'loop'):
        plans = [_engine.IirPlan([f], n, 1) for f in filt]
        xs_, ys_ = x.stride(0) * 8, y.stride(0) * 8
        xp, yp = x.data_ptr(), y.data_ptr()

        def loop():
            for i, p in enumerate(plans):
                p.apply(xp + i * xs_, n, yp + i * ys_, n, None, None, 0.0, stream)
        r['loop_ms'] = round(timed(loop, max(3, reps // 4), warm=1), 4)
        r['loop_gbs'] = gbs(r['loop_ms'])
        for p in plans:
            p.close()
    if 'rows_ms' in r and 'shared_ms' in r:
        r['rows_over_shared'] = round(r['rows_ms'] / r['shared_ms'], 3)
    if 'rows_ms' in r and 'loop_ms' in r:
        r['loop_over_rows'] = round(r['loop_ms'] / r['rows_ms'], 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='awg,256x1e7,8x1e7')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', choices=['rows', 'shared', 'loop'], help='one leg only (profiler runs)')
    ap.add_argument('--json')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    ap.add_argument('--limit', type=int, default=240, help='seconds per shape')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_shape(a.child, a.reps, a.only)), flush=True)
        return 0
    res = []
    for name in a.shapes.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', name, '--reps', str(a.reps)]
        if a.only:
            cmd += ['--only', a.only]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f'{name}: no result within {a.limit} s; stopping', file=sys.stderr)
            return 1
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print(f'{name}: exit status {p.returncode}; stopping', file=sys.stderr)
            return 1
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        res.append(json.loads(line))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
