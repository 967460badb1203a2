#!/usr/bin/env python3
"""The sampler that writes DAC codes itself (distortion.SampledDac: wfk_sample_short_dac) against the two launches it
replaces, in ONE process on the same card, the forms alternating:

    python tools/sampled_dac_bench.py [--cases awg,awg64,duty30,flat_top] [--reps 20] [--json profiles/....json]

  (a) fused          SampledDac.launch_torch(codes): one kernel, 2 B/sample of HBM traffic
  (b) fused+counts   the same with the clip report
  (c) two            BatchSampler.launch_torch(z) (float64) followed by DacStage.apply_torch(z, codes): 18 B/sample
  (d) sampler        BatchSampler.launch_torch(z) alone: the float64 launch the fused kernel shares its arithmetic with
  cases  awg       2048 x 1e5 at 2 GS/s, workloads.awg_channel rows      awg64    64 x 1e5 of the same
         duty30    2048 x 1e5, the 30 % duty variant (pure-fill units)   flat_top 2048 x 1e5 awg_shape_channel flat_top
ms = median of --reps device-event timings after a warm-up, the forms taken in turn (a, b, c, d, a, ...).  The
yardstick is (c) of the same run; codes and counts of (b) and (c) are compared bit for bit."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'awg': ('awg', 2048, 10**5), 'awg64': ('awg', 64, 10**5), 'duty30': ('duty30', 2048, 10**5),
         'flat_top': ('flat_top', 2048, 10**5)}
RATE = 2e9
DISTINCT = 16        # distinct waveforms, tiled up to the batch (the device tables of every copy are its own)


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
    if kind == 'flat_top':
        chans = [wl.awg_shape_channel(wf, 'flat_top', c, n, RATE) for c in range(distinct)]
    else:
        chans = [wl.awg_channel(wf, c, n, RATE, kind == 'duty30') for c in range(distinct)]
    grid, tile = wl.awg_grid(n, RATE), rows // distinct
    dev = torch.device('cuda', 0)
    z = torch.empty((rows, n), dtype=torch.float64, device=dev)
    codes, codes2 = (torch.empty((rows, n), dtype=torch.int16, device=dev) for _ in range(2))
    counts, counts2 = (torch.empty((rows, 3), dtype=torch.int64, device=dev) for _ in range(2))
    fused = distortion.SampledDac.from_full_scale(chans, grid, 0.8, tile=tile)        # a few percent of the samples clip
    sampler = BatchSampler(chans, grid, tile=tile)
    stage = distortion.DacStage.from_full_scale(0.8, n, batch=rows)

    def two():
        sampler.launch_torch(z)
        stage.apply_torch(z, codes2, counts2)
    forms = {'fused': lambda: fused.launch_torch(codes), 'fused_counts': lambda: fused.launch_torch(codes, counts),
             'two': two, 'sampler': lambda: sampler.launch_torch(z)}
    for _ in range(3):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            t[k].append(event_ms(f))
    forms['fused_counts']()
    two()
    torch.cuda.synchronize()
    ms = {k: float(np.median(v)) for k, v in t.items()}
    r = dict(case=name, rows=rows, n=n, fused=bool(fused.fused), why_not=fused.why_not,
             fused_kernel=fused.kernel_name(), two_kernels=sampler.plan.kernel_name(np.float64) + ' + ' + stage.kernel_name(True),
             fused_ms=round(ms['fused'], 4), fused_counts_ms=round(ms['fused_counts'], 4), two_ms=round(ms['two'], 4),
             sampler_f64_ms=round(ms['sampler'], 4), two_over_fused=round(ms['two'] / ms['fused'], 3),
             fused_over_sampler=round(ms['fused'] / ms['sampler'], 3),
             fused_min_ms=round(min(t['fused']), 4), two_min_ms=round(min(t['two']), 4),
             codes_equal=bool(torch.equal(codes, codes2)), counts_equal=bool(torch.equal(counts, counts2)),
             clipped=int(counts2[:, :2].sum()))
    fused.close()
    sampler.close()
    stage.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='awg,awg64,duty30,flat_top')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for name in a.cases.split(','):
        res.append(run_case(name, a.reps))
        print(json.dumps(res[-1]), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    return 0 if all(r['codes_equal'] and r['counts_equal'] for r in res) else 1


if __name__ == '__main__':
    sys.exit(main())
