#!/usr/bin/env python3
"""Sampler inside the per-row IIR stage (distortion.SampledIirRows: iir_rows_short / iir_rows_sampled) against what
the tree offered for the same job before it, in ONE process per case on the same card, alternating:

    python tools/iir_rows_chain_bench.py [--cases awg,fine,awg64] [--reps 20] [--json profiles/....json]

  (a) fused    SampledIirRows.launch_torch(z): one kernel, 8 B/sample of HBM traffic (the output)
  (b) two      BatchSampler.launch_torch(z) followed by IirStage([...one cascade per row...]).apply_torch(z) in place:
               24 B/sample (the sampler writes x, iir_rows_tile reads it back and writes y)
  cases  awg    2048 x 1e5 at 2 GS/s, workloads.awg_channel rows (the short fill)
         fine   256 x 1e6 on a fine grid, workloads.sum_channel rows (the lean fill)
         awg64  64 x 1e5 at 2 GS/s: a quarter of the chip's 256 CUs has a row to walk
Every case is fp64 with three first-order sections per row, all rows different.  ms = median of --reps device-event
timings after a warm-up, the two forms taken in turn (fused, two, fused, two, ...); roof = output bytes / ms / 8 TB/s.
The two forms' outputs are compared on a few rows.  Every case runs in a child process of its own under a time limit;
the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
CASES = {'awg': ('awg', 2048, 10**5), 'fine': ('fine', 256, 10**6), 'awg64': ('awg', 64, 10**5)}
RATE = 2e9
DISTINCT = 64        # distinct waveforms, tiled up to the batch (the device tables of every copy are its own)


def row_cascades(rows, seed=0):
    """three first-order exp-decay corrections per row, all rows different"""
    from waveforms_amd import distortion
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rows):
        taus = [rng.uniform(20e-9, 40e-9), rng.uniform(80e-9, 200e-9), rng.uniform(0.5e-6, 5e-6)]
        amps = rng.uniform(0.005, 0.03, 3) * rng.choice([-1, 1], 3)
        out.append([distortion.exp_decay_filter(A, t, RATE) for A, t in zip(amps, taus)])
    return out


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_case(name, reps):
    import torch
    import waveforms_amd as wf
    from waveforms_amd import distortion, workloads as wl
    from waveforms_amd._sampling import BatchSampler
    kind, rows, n = CASES[name]
    distinct = min(DISTINCT, rows)
    if kind == 'awg':
        chans = [wl.awg_channel(wf, c, n, RATE) for c in range(distinct)]
        grid = wl.awg_grid(n, RATE)
    else:
        nseg = n // 2000                                       # ~2000 samples per pulse, as the FIR / IIR chain benches
        chans = [wl.sum_channel(wf, nseg, 1000 + c) for c in range(distinct)]
        grid = ('linspace', 0.0, nseg * wl.SPAN, n, False)
    tile = rows // distinct
    secs = row_cascades(rows)
    dev = torch.device('cuda', 0)
    z = torch.empty((rows, n), dtype=torch.float64, device=dev)
    z2 = torch.empty_like(z)
    fused = distortion.SampledIirRows(chans, grid, secs, tile=tile)
    sampler = BatchSampler(chans, grid, tile=tile)
    stage = distortion.IirStage(secs, n, rows)

    def two():
        sampler.launch_torch(z2)
        stage.apply_torch(z2)
    one = lambda: fused.launch_torch(z)
    for _ in range(3):
        one()
        two()
    torch.cuda.synchronize()
    t1, t2, ts = [], [], []
    for _ in range(reps):
        t1.append(event_ms(one))
        t2.append(event_ms(two))
    for _ in range(max(3, reps // 4)):                         # the sampler's share of the two launches
        ts.append(event_ms(lambda: sampler.launch_torch(z2)))
    stage.apply_torch(z2)
    torch.cuda.synchronize()
    probe = sorted({0, rows // 2, rows - 1})
    a, b = z[probe].cpu().numpy(), z2[probe].cpu().numpy()
    out_bytes = rows * n * 8
    ms1, ms2 = float(np.median(t1)), float(np.median(t2))
    r = dict(case=name, rows=rows, n=n, dtype='float64', sections_per_row=3, fused=bool(fused.fused),
             fused_kernel=fused.kernel_name(), why_not=fused.why_not,
             two_kernels=sampler.plan.kernel_name(np.float64) + ' + ' + stage.kernel_name(),
             fused_ms=round(ms1, 4), two_ms=round(ms2, 4), sampler_alone_ms=round(float(np.median(ts)), 4),
             fused_min_ms=round(min(t1), 4), two_min_ms=round(min(t2), 4),
             two_over_fused=round(ms2 / ms1, 3),
             fused_roof=round(out_bytes / (ms1 * 1e-3) / HBM_BYTES_PER_S, 3),
             two_roof=round(out_bytes / (ms2 * 1e-3) / HBM_BYTES_PER_S, 3),
             max_abs_diff_fused_vs_two=float('%.3g' % np.max(np.abs(a - b))), peak=float('%.3g' % np.abs(b).max()))
    fused.close()
    sampler.close()
    stage.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='awg,fine,awg64')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    ap.add_argument('--limit', type=int, default=240, help='seconds per case')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_case(a.child, a.reps)), flush=True)
        return 0
    res = []
    for name in a.cases.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', name, '--reps', str(a.reps)]
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
