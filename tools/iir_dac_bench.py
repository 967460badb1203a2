#!/usr/bin/env python3
"""The per-row IIR stage that ends in DAC codes (distortion.IirDacStage: iir_rows_dac; distortion.SampledIirDac:
iir_rows_short_dac / iir_rows_sampled_dac) timed with device events next to what it replaces, in ONE process on one
card, on the same tensors, the legs taken in turn:

    python tools/iir_dac_bench.py [--shapes 2048x100000,256x10000000] [--dtypes f64,f32] [--sampled awg,fine]
                                  [--reps 20] [--json profiles/....json]

  stage legs, per shape and dtype, one section of order 3 per row (all rows different), with counts:
    fused  IirDacStage.apply_torch(x, codes, counts): one kernel, sizeof(T) + 2 B/sample (10 fp64, 6 fp32)
    two    IirStage.apply_torch(x, out=y) then DacStage.apply_torch(y, codes, counts): 2 sizeof(T) + sizeof(T) + 2
           B/sample (26 fp64, 14 fp32) -- the yardstick, both stages as the tree has them
  sampled legs (fp64), three first-order sections per row:
    fused  SampledIirDac.launch_torch(codes, counts): one kernel, 2 B/sample
    two    SampledIirRows.launch_torch(z) then DacStage.apply_torch(z, codes, counts): 8 + 8 + 2 B/sample
    cases  awg   2048 x 1e5 at 2 GS/s, workloads.awg_channel rows (the short fill)
           fine  256 x 1e6 on a fine grid, workloads.sum_channel rows (the lean fill)

Every leg: 3 warm-up runs, then --reps event-timed runs of fused, two, fused, two, ...; reported are the median, the
minimum and the maximum of each.  GB/s: the fused form's own bytes (its accounting above) over its median.  Before
timing the fused codes and counts are compared with the two launches': they must be equal."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from waveforms_amd import distortion  # noqa: E402

RATE = 2e9
DISTINCT = 64        # distinct waveforms, tiled up to the batch
SAMPLED = {'awg': ('awg', 2048, 10**5), 'fine': ('fine', 256, 10**6)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(one, two, reps):
    """-> ({median, min, max} of `one`, of `two`) in ms"""
    for _ in range(3):
        one()
        two()
    torch.cuda.synchronize()
    t1, t2 = [], []
    for _ in range(reps):
        t1.append(event_ms(one))
        t2.append(event_ms(two))
    stat = lambda t: dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))
    return stat(t1), stat(t2)


def order3_rows(rows, seed=0):
    """one section of order 3 per row: three exp-decay corrections combined, all rows different"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rows):
        taus = [rng.uniform(20e-9, 40e-9), rng.uniform(80e-9, 200e-9), rng.uniform(0.5e-6, 5e-6)]
        amps = rng.uniform(0.005, 0.03, 3) * rng.choice([-1, 1], 3)
        out.append([distortion.combine_filters([distortion.exp_decay_filter(A, t, RATE) for A, t in zip(amps, taus)])])
    return out


def first_order_rows(rows, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rows):
        taus = [rng.uniform(20e-9, 40e-9), rng.uniform(80e-9, 200e-9), rng.uniform(0.5e-6, 5e-6)]
        amps = rng.uniform(0.005, 0.03, 3) * rng.choice([-1, 1], 3)
        out.append([distortion.exp_decay_filter(A, t, RATE) for A, t in zip(amps, taus)])
    return out


def result(kind, rows, n, fused_bytes, two_bytes, f, t, equal, **more):
    r = dict(leg=kind, rows=rows, n=n, equal_to_two_launches=equal, fused_ms=f['median'], fused_min_ms=f['min'],
             fused_max_ms=f['max'], two_ms=t['median'], two_min_ms=t['min'], two_max_ms=t['max'],
             two_over_fused=round(t['median'] / f['median'], 3),
             # outside the spread of the legs: the slowest fused run against the fastest run of the two launches
             fused_not_slower=bool(f['max'] <= t['min'] or f['median'] <= t['median']),
             fused_bytes_per_sample=fused_bytes, two_bytes_per_sample=two_bytes,
             fused_GBps=round(fused_bytes * rows * n / f['median'] / 1e6, 1),
             two_GBps=round(two_bytes * rows * n / t['median'] / 1e6, 1))
    r.update(more)
    return r


def stage_leg(kind, rows, n, reps):
    dtype, tdt = (np.float64, torch.float64) if kind == 'f64' else (np.float32, torch.float32)
    dev = torch.device('cuda', 0)
    secs = order3_rows(rows)
    rng = np.random.default_rng(1)
    gain, offset = np.full(rows, 30000.0) * rng.choice([-1, 1], rows), rng.uniform(-3.0, 3.0, rows)   # +-1.09 clips
    x = torch.rand(rows, n, dtype=tdt, device=dev) * 2.2 - 1.1
    y = torch.empty_like(x)
    codes = torch.empty((rows, n), dtype=torch.int16, device=dev)
    codes2 = torch.empty_like(codes)
    counts, counts2 = (torch.empty((rows, 3), dtype=torch.int64, device=dev) for _ in range(2))
    fu = distortion.IirDacStage(secs, n, gain, offset=offset, dtype=dtype)
    iir = distortion.IirStage(secs, n, rows, dtype=dtype)
    dac = distortion.DacStage(gain, n, offset=offset, dtype=dtype, batch=rows)

    def fused():
        fu.apply_torch(x, codes, counts)

    def two():
        iir.apply_torch(x, out=y)
        dac.apply_torch(y, codes2, counts2)

    fused()
    two()
    torch.cuda.synchronize()
    equal = bool(torch.equal(codes, codes2)) and bool(torch.equal(counts, counts2))
    f, t = alternate(fused, two, reps)
    es = np.dtype(dtype).itemsize
    r = result('stage', rows, n, es + 2, 3 * es + 2, f, t, equal, dtype=kind, kernel=fu.kernel_name(),
               two_kernels=iir.kernel_name() + ' + ' + dac.kernel_name(True), clipped=int(counts[:, :2].sum()))
    for st in (fu, iir, dac):
        st.close()
    del x, y, codes, codes2
    torch.cuda.empty_cache()
    return r


def sampled_leg(name, reps):
    import waveforms_amd as wf
    from waveforms_amd import workloads as wl
    kind, rows, n = SAMPLED[name]
    distinct = min(DISTINCT, rows)
    if kind == 'awg':
        chans = [wl.awg_channel(wf, c, n, RATE) for c in range(distinct)]
        grid = wl.awg_grid(n, RATE)
    else:
        nseg = n // 2000
        chans = [wl.sum_channel(wf, nseg, 1000 + c) for c in range(distinct)]
        grid = ('linspace', 0.0, nseg * wl.SPAN, n, False)
    tile = rows // distinct
    secs = first_order_rows(rows)
    rng = np.random.default_rng(1)
    gain, offset = np.full(rows, 30000.0) * rng.choice([-1, 1], rows), rng.uniform(-3.0, 3.0, rows)
    dev = torch.device('cuda', 0)
    z = torch.empty((rows, n), dtype=torch.float64, device=dev)
    codes = torch.empty((rows, n), dtype=torch.int16, device=dev)
    codes2 = torch.empty_like(codes)
    counts, counts2 = (torch.empty((rows, 3), dtype=torch.int64, device=dev) for _ in range(2))
    fu = distortion.SampledIirDac(chans, grid, secs, gain, offset=offset, tile=tile)
    sr = distortion.SampledIirRows(chans, grid, secs, tile=tile)
    dac = distortion.DacStage(gain, n, offset=offset, batch=rows)

    def fused():
        fu.launch_torch(codes, counts)

    def two():
        sr.launch_torch(z)
        dac.apply_torch(z, codes2, counts2)

    fused()
    two()
    torch.cuda.synchronize()
    equal = bool(torch.equal(codes, codes2)) and bool(torch.equal(counts, counts2))
    f, t = alternate(fused, two, reps)
    r = result('sampled', rows, n, 2, 18, f, t, equal, case=name, dtype='f64', fused=bool(fu.fused), why_not=fu.why_not,
               kernel=fu.kernel_name(), two_kernels=sr.kernel_name() + ' + ' + dac.kernel_name(True),
               clipped=int(counts[:, :2].sum()))
    for st in (fu, sr, dac):
        st.close()
    del z, codes, codes2
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='2048x100000,256x10000000')
    ap.add_argument('--dtypes', default='f64,f32')
    ap.add_argument('--sampled', default='awg,fine')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('iir_dac_bench: no GPU')
    res = []
    for shape in [s for s in a.shapes.split(',') if s]:
        rows, n = (int(v) for v in shape.split('x'))
        for kind in a.dtypes.split(','):
            res.append(stage_leg(kind, rows, n, a.reps))
            print(json.dumps(res[-1]), flush=True)
    for name in [s for s in a.sampled.split(',') if s]:
        res.append(sampled_leg(name, a.reps))
        print(json.dumps(res[-1]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
