#!/usr/bin/env python3
"""Per-row shift (distortion.ShiftStage, csrc/wfk_shift_rows.hip) timed with device events, next to two yardsticks:
`out.copy_(x)` on the very same tensors in the same process (the same 16 B/sample of traffic, no arithmetic), and
the only route the tree had for rows before the stage: a Python loop of `distortion.shift(row, delay, dt)`, each call
an upload, a 3-tap FIR, a download and a host shift.

    python tools/shift_rows_bench.py [--cases S1,S3] [--reps 20] [--loop-rows 8] [--json out.json]

fp64, every row its own fractional delay of either sign.  One line per case: ms per apply and per copy (median, min
and max of --reps event-timed runs after a warm-up; the two are timed alternately, a block of each), their ratio,
GB/s of the apply, and the host loop: seconds per row (median over --loop-rows rows) times the number of rows.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd import distortion  # noqa: E402

CASES = {   # name: (rows, n)
    'S1': (2048, 10**5),
    'S2': (256, 10**6),
    'S3': (8, 10**7),
}
DT = 1 / 2e9


def timed(fn, reps, warm=3):
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
    return dict(median=round(float(np.median(ts)), 4), min=round(float(min(ts)), 4), max=round(float(max(ts)), 4))


def run_case(name, reps, loop_rows):
    rows, n = CASES[name]
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    delays = rng.uniform(-200.0, 200.0, rows) * DT
    x = torch.randn(rows, n, dtype=torch.float64, device=dev)
    y = torch.empty_like(x)
    st = distortion.ShiftStage(delays, n, DT)
    apply_a = timed(lambda: st.apply_torch(x, y), reps)
    copy_a = timed(lambda: y.copy_(x), reps)
    apply_b = timed(lambda: st.apply_torch(x, y), reps)
    copy_b = timed(lambda: y.copy_(x), reps)
    st.apply_torch(x, y)
    # parity of a few rows against the closed form, at the size that is timed
    err = 0.0
    for r in np.unique(np.r_[0, rows - 1, rng.integers(0, rows, 2)]):
        xr, p, d = x[r].cpu().numpy(), int(st.points[r]), float(st.deltas[r])
        s = (1 - d) * xr + d * np.r_[0.0, xr[:-1]] if d > 0 else xr
        want = np.zeros(n)
        if 0 <= p < n:
            want[p:] = s[:n - p]
        elif -n < p < 0:
            want[:n + p] = s[-p:]
        err = max(err, float(np.max(np.abs(y[r].cpu().numpy() - want))))
    kernel = st.kernel_name()
    st.close()
    # the host loop: per-row time from a few rows, both copies included
    xs = [x[r].cpu().numpy() for r in range(min(rows, loop_rows))]
    distortion.shift(xs[0], delays[0], DT)
    per_row = []
    for r, xr in enumerate(xs):
        t0 = time.perf_counter()
        distortion.shift(xr, delays[r], DT)
        per_row.append(time.perf_counter() - t0)
    loop_ms = float(np.median(per_row)) * rows * 1e3
    ms = min(apply_a['median'], apply_b['median'])
    cp = min(copy_a['median'], copy_b['median'])
    r = dict(case=name, rows=rows, n=n, kernel=kernel, apply_ms=[apply_a, apply_b], copy_ms=[copy_a, copy_b],
             apply_over_copy=round(ms / cp, 4), apply_GBps=round(2 * rows * n * 8 / ms / 1e6, 1),
             copy_GBps=round(2 * rows * n * 8 / cp / 1e6, 1), host_loop_ms=round(loop_ms, 2),
             host_loop_rows_timed=len(xs), speedup=round(loop_ms / ms, 1), max_abs_err=float('%.3g' % err),
             bytes=2 * rows * n * 8)
    del x, y
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='S1,S2,S3')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--loop-rows', type=int, default=8)
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for name in a.cases.split(','):
        r = run_case(name, a.reps, a.loop_rows)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
