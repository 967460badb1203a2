#!/usr/bin/env python3
"""Per-row reflection correction (distortion.ReflectionStage) timed with device events, next to the only route the
tree had for per-row parameters before it: a Python loop of `correct_reflection(row, A_r, tau_r, fs)`, each call
building H on the host, uploading it and the row, and downloading the result.

    python tools/spectral_rows_bench.py [--cases S1,S3] [--reps 20] [--loop-rows 8] [--json out.json]

fp64, one `correct` term per row, every row its own (A, tau).  One line per case: ms per apply (median of --reps
after a warm-up), the same with a term-free stage (the transforms, the copies and a plain scale: what an apply costs
without the synthesis), ms of a plain complex multiply over the same spectrum bytes (torch, in place: the floor
of a pass that reads H instead of forming it), the bytes each pass of an apply moves, and the host loop: seconds per
row (median over --loop-rows rows) times the number of rows.
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
    'S3': (1, 10**7),
}
FS = 2e9


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
    return float(np.median(ts))


def run_case(name, reps, loop_rows):
    rows, n = CASES[name]
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    A, tau = rng.uniform(-0.3, 0.3, rows), rng.uniform(1e-9, 200e-9, rows)
    x = torch.randn(rows, n, dtype=torch.float64, device=dev)
    y = torch.empty_like(x)
    nf = n // 2 + 1
    st = distortion.ReflectionStage([[('correct', a, t)] for a, t in zip(A, tau)], n, FS)
    ms = timed(lambda: st.apply_torch(x, out=y), reps)
    # parity of a few rows against the host formula, at the size that is timed
    pick = np.unique(np.r_[0, rows - 1, rng.integers(0, rows, 2)])
    f = np.fft.rfftfreq(n, 1 / FS)
    err = 0.0
    for r in pick:
        xr = x[r].cpu().numpy()
        want = np.fft.irfft(np.fft.rfft(xr) / distortion.reflection_filter(f, A[r], tau[r]), n)
        err = max(err, float(np.max(np.abs(y[r].cpu().numpy() - want)) / max(1.0, np.abs(xr).max())))
    st.close()
    plain = distortion.ReflectionStage([[] for _ in range(rows)], n, FS)
    ms_plain = timed(lambda: plain.apply_torch(x, out=y), reps)
    plain.close()
    spec = torch.randn(rows, nf, dtype=torch.complex128, device=dev)
    H = torch.randn(rows, nf, dtype=torch.complex128, device=dev)
    ms_mul = timed(lambda: spec.mul_(H), reps)
    del spec, H
    # the host loop: per-row time from a few rows, host H and both copies included
    xs = [x[r].cpu().numpy() for r in range(min(rows, loop_rows))]
    distortion.correct_reflection(xs[0], A[0], tau[0], FS)
    per_row = []
    for r, xr in enumerate(xs):
        t0 = time.perf_counter()
        distortion.correct_reflection(xr, A[r], tau[r], FS)
        per_row.append(time.perf_counter() - t0)
    loop_ms = float(np.median(per_row)) * rows * 1e3
    sig_b, spec_b = rows * n * 8, rows * nf * 16
    r = dict(case=name, rows=rows, n=n, apply_ms=round(ms, 4), apply_no_terms_ms=round(ms_plain, 4),
             torch_complex_mul_ms=round(ms_mul, 4), host_loop_ms=round(loop_ms, 2),
             host_loop_rows_timed=len(xs), speedup=round(loop_ms / ms, 1), max_rel_err=float('%.3g' % err),
             bytes=dict(stage_copy=2 * sig_b, r2c=sig_b + spec_b, spec_rows_mul=2 * spec_b, c2r=spec_b + sig_b))
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
