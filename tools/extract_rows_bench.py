#!/usr/bin/env python3
"""Per-row kernel extraction (distortion.KernelExtractor, csrc/wfk_extract_rows.hip) timed with device events, with
and without smoothing (M = 40 taps), next to two yardsticks: `out.copy_(x)` on tensors of the result's shape (what the
tap-free last pass, extract_smooth's copy body, has to move), and the route the tree had before the stage: a Python
loop of host `distortion.extractKernel(sig_in[r], sig_out[r], ...)`, timed on --loop-rows rows and scaled.

    python tools/extract_rows_bench.py [--cases S1,S3] [--reps 20] [--loop-rows 8] [--json out.json] [--profile-reps N]

fp64, every row its own pair of signals (the recipe of tests/cases.extract_input, drawn on the device).  One line per
case: ms per apply without and with taps (median, min and max of --reps event-timed runs after a warm-up), ms per
copy, the host loop, and the parity of a few rows against the host function at the size that is timed.
--profile-reps N: no timing, N applies of each form and nothing else (what `rocprofv3 --kernel-trace --stats -- python
tools/extract_rows_bench.py --cases S1 --profile-reps 13` is pointed at: a run of its own per shape, which gives the
share of extract_ratio and extract_smooth in an apply; extract_ratio moves 3Z = 3 * rows * (n/2 + 1) * 16 B).
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
    'S3': (8, 10**6),
}
FS = 2e9
M = 40
BW = 2 * FS / (M + 0.5)


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


def signals(rows, n, dev):
    """sig_in: a random walk plus noise; sig_out: its image under 0.3 delta + a 24-tap decay (truncated, causal)"""
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.randn(rows, n, dtype=torch.float64, device=dev, generator=g)
    a += torch.cumsum(torch.randn(rows, n, dtype=torch.float64, device=dev, generator=g), dim=1) / 20
    k = np.exp(-np.arange(24) / 5.0)
    k /= k.sum()
    k[0] += 0.3
    b = torch.zeros_like(a)
    for d, kd in enumerate(k):
        b[:, d:] += float(kd) * a[:, :n - d]
    return a, b


def run_case(name, reps, loop_rows, profile_reps):
    rows, n = CASES[name]
    dev = torch.device('cuda', 0)
    a, b = signals(rows, n, dev)
    plain = distortion.KernelExtractor(n, rows, FS)
    smooth = distortion.KernelExtractor(n, rows, FS, BW)
    assert smooth.taps is not None and len(smooth.taps) == M
    out = torch.empty((rows, n), dtype=torch.float64, device=dev)
    if profile_reps:
        for _ in range(profile_reps):
            plain.apply_torch(a, b, out)
        for _ in range(profile_reps):
            smooth.apply_torch(a, b, out)
        torch.cuda.synchronize()
        plain.close()
        smooth.close()
        return dict(case=name, rows=rows, n=n, profile_reps=profile_reps)
    t_plain = timed(lambda: plain.apply_torch(a, b, out), reps)
    t_copy = timed(lambda: out.copy_(a), reps)
    t_smooth = timed(lambda: smooth.apply_torch(a, b, out), reps)
    # parity of a few rows against the host function, at the size that is timed
    pick = sorted({0, rows - 1, rows // 2})
    err = {}
    for label, ex, bw in (('plain', plain, None), ('smooth', smooth, BW)):
        got = ex.apply_torch(a, b, out).index_select(0, torch.tensor(pick, device=dev)).cpu().numpy()
        worst = 0.0
        for g_row, r in zip(got, pick):
            want = distortion.extractKernel(a[r].cpu().numpy(), b[r].cpu().numpy(), FS, bw)
            worst = max(worst, float(np.max(np.abs(g_row - want)) / np.max(np.abs(want))))
        err[label] = float('%.3g' % worst)
    kernel = plain.kernel_name()
    plain.close()
    smooth.close()
    # the host loop: per-row time from a few rows
    loop = {}
    pairs = [(a[r].cpu().numpy(), b[r].cpu().numpy()) for r in range(min(rows, loop_rows))]
    for label, bw in (('plain', None), ('smooth', BW)):
        distortion.extractKernel(*pairs[0], FS, bw)
        per_row = []
        for ar, br in pairs:
            t0 = time.perf_counter()
            distortion.extractKernel(ar, br, FS, bw)
            per_row.append(time.perf_counter() - t0)
        loop[label] = round(float(np.median(per_row)) * rows * 1e3, 2)
    S, Z = rows * n * 8, rows * (n // 2 + 1) * 16
    r = dict(case=name, rows=rows, n=n, taps=M, kernel=kernel, apply_plain_ms=t_plain, apply_smooth_ms=t_smooth,
             copy_ms=t_copy, host_loop_ms=loop, host_loop_rows_timed=len(pairs),
             speedup_plain=round(loop['plain'] / t_plain['median'], 1),
             speedup_smooth=round(loop['smooth'] / t_smooth['median'], 1),
             rel_err_vs_host=err, S_bytes=S, Z_bytes=Z, ratio_bytes=3 * Z, smooth_bytes=2 * S)
    del a, b, out
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='S1,S2,S3')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--loop-rows', type=int, default=8)
    ap.add_argument('--profile-reps', type=int, default=0)
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for name in a.cases.split(','):
        r = run_case(name, a.reps, a.loop_rows, a.profile_reps)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
