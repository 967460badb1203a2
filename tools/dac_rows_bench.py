#!/usr/bin/env python3
"""The DAC stage (distortion.DacStage, csrc/wfk_dac_rows.hip) timed with device events, next to two yardsticks on
the same box and the very same tensors in the same process:

  * the torch chain it replaces, `torch.clamp(torch.round(x * g + o), lo, hi).to(torch.int16)`: five elementwise
    passes (the chain rounds half to even as the stage does, has no NaN rule and counts nothing);
  * `y.copy_(x)`, a plain copy of the input rows: the stream ceiling (it moves 2 * sizeof(sample) per sample, the
    stage sizeof(sample) + 2).

    python tools/dac_rows_bench.py [--cases D1,D2] [--legs f64,f64c,f32,f32c,f64k2,f64k2c] [--reps 20] [--json out.json]

Cases: D1 = 256 x 1e7, D2 = 2048 x 1e5.  Legs: float64 / float32 rows, `c` = with the clip report, `k2` = I/Q pairs
interleaved.  One line per case and leg: ms per apply, per chain and per copy (median, min and max of --reps
event-timed runs after a warm-up; the three are timed alternately, two blocks of each), GB/s of the stage against
its traffic floor (10 B per float64 sample, 6 B per float32 sample), of the copy, and the ratios.  The codes of a few
rows are compared with the chain's at the size that is timed (NaN-free input: the chain has no rule for NaN).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd import distortion  # noqa: E402

CASES = {   # name: (rows, n)
    'D1': (256, 10**7),
    'D2': (2048, 10**5),
}
LEGS = {    # name: (dtype, counts, interleave)
    'f64': (np.float64, False, 1), 'f64c': (np.float64, True, 1),
    'f32': (np.float32, False, 1), 'f32c': (np.float32, True, 1),
    'f64k2': (np.float64, False, 2), 'f64k2c': (np.float64, True, 2),
}


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


def run_leg(case, leg, reps):
    rows, n = CASES[case]
    dtype, with_counts, k = LEGS[leg]
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    hi, lo = 32767, -32768
    gain = rng.uniform(0.9, 1.0, rows) * hi * np.where(np.arange(rows) % 3 == 1, -1.0, 1.0)
    offset = rng.uniform(-50.0, 50.0, rows)
    x = torch.rand(rows, n, dtype=tdt, device=dev) * 2.1 - 1.05          # a few percent past each rail
    y = torch.empty_like(x)
    st = distortion.DacStage(gain, n, offset=offset, interleave=k, dtype=dtype)
    out = torch.empty((st.out_rows, st.out_n), dtype=torch.int16, device=dev)
    counts = torch.empty((rows, 3), dtype=torch.int64, device=dev) if with_counts else None
    g = torch.from_numpy(gain).to(dev)[:, None]
    o = torch.from_numpy(offset).to(dev)[:, None]

    def stage():
        st.apply_torch(x, out, counts)

    def chain():
        return torch.clamp(torch.round(x * g + o), lo, hi).to(torch.int16)

    def copy():
        y.copy_(x)

    t = {name: [] for name in ('stage', 'chain', 'copy')}
    for _ in range(2):
        for name, fn in (('stage', stage), ('chain', chain), ('copy', copy)):
            t[name].append(timed(fn, reps))
    # parity with the chain on a few rows, at the size that is timed (float32 rows: the chain promotes to float64
    # through g, as the stage widens)
    stage()
    want = chain()
    got = out.view(st.out_rows, n, k).permute(0, 2, 1).reshape(rows, n) if k == 2 else out
    pick = torch.from_numpy(np.unique(np.r_[0, rows - 1, rng.integers(0, rows, 2)])).to(dev)
    differ = int((got[pick] != want[pick]).sum())
    clipped = None if counts is None else [int(v) for v in counts.sum(dim=0).cpu()]
    kernel = st.kernel_name(with_counts)
    st.close()
    ms, ch, cp = (min(b['median'] for b in t[name]) for name in ('stage', 'chain', 'copy'))
    es = np.dtype(dtype).itemsize
    floor_bytes, copy_bytes = rows * n * (es + 2), rows * n * 2 * es
    r = dict(case=case, leg=leg, rows=rows, n=n, interleave=k, counts=with_counts, kernel=kernel,
             stage_ms=t['stage'], chain_ms=t['chain'], copy_ms=t['copy'],
             stage_GBps=round(floor_bytes / ms / 1e6, 1), copy_GBps=round(copy_bytes / cp / 1e6, 1),
             stage_over_copy=round(ms / cp, 4), stage_rate_over_copy_rate=round(floor_bytes / ms / (copy_bytes / cp), 4),
             chain_over_stage=round(ch / ms, 2), floor_bytes=floor_bytes, codes_differ_from_chain=differ,
             clipped_below_above_nan=clipped)
    del x, y, out, want, got
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='D1,D2')
    ap.add_argument('--legs', default=','.join(LEGS))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for case in a.cases.split(','):
        for leg in a.legs.split(','):
            r = run_leg(case, leg, a.reps)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
