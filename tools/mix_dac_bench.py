#!/usr/bin/env python3
"""The fused mix-to-codes stage (distortion.MixDacStage, csrc/wfk_mix_dac.hip) timed with device events next to what it
replaces, on the same box and the very same tensors in the same process:

  * fused: `MixDacStage.apply_torch(x, codes[, counts])`, one kernel;
  * two:   `MixStage.apply_torch(x, y)` then `DacStage.apply_torch(y, codes[, counts])`, two launches with the float
           rows y between them -- the yardstick;
  * dac:   `DacStage.apply_torch(y, codes[, counts])` alone.

    python tools/mix_dac_bench.py [--cases iq,tri,band4,dense] [--dtypes f64,f32] [--shapes 256x1000000,2048x100000]
                                  [--reps 20] [--json out.json]

Cases on rows x n samples: iq = 2 x 2 blocks with interleave 2, tri = tridiagonal and band4 = a band of half-width 4
with interleave 1, dense = rows x rows (not the stage's shape: 256 x 1e5 only, one line).  Every case with and without
counts.  The three legs are timed alternately, two blocks of each, every block 3 warm-up and --reps event-timed runs;
a leg's figure is the LOWER median of its two blocks and its spread the distance between the two medians.  GB/s on the
fused stage's traffic model, (reads * n * sizeof(sample) + 2 * rows_out * n) bytes.  Before timing, the fused codes and
counts are compared with the two launches': they must be equal."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd import distortion  # noqa: E402


def band(rows, k, rng):
    m = np.zeros((rows, rows))
    for d in range(-k, k + 1):
        idx = np.arange(max(0, -d), min(rows, rows - d))
        m[idx, idx + d] = (1.0 if d == 0 else 0.0) + 0.03 * rng.uniform(0.2, 1.0, len(idx))
    return m


def matrix_of(case, rows, rng):
    """-> (matrix, interleave)"""
    if case == 'iq':
        m = np.zeros((rows, rows))
        for p in range(rows // 2):
            m[2 * p:2 * p + 2, 2 * p:2 * p + 2] = np.eye(2) + 0.05 * rng.standard_normal((2, 2))
        return m, 2
    if case == 'tri':
        return band(rows, 1, rng), 1
    if case == 'band4':
        return band(rows, 4, rng), 1
    if case == 'dense':
        return rng.uniform(0.1, 1.0, (rows, rows)) / rows, 1
    raise SystemExit(f'unknown case {case}')


def block(fn, reps, warm=3):
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


def run_leg(case, kind, rows, n, with_counts, reps):
    dtype = np.float64 if kind == 'f64' else np.float32
    tdt = torch.float64 if kind == 'f64' else torch.float32
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    m, k = matrix_of(case, rows, rng)
    mix_offset = rng.uniform(-0.01, 0.01, rows)
    gain, dac_offset = np.full(rows, 30000.0), rng.uniform(-3.0, 3.0, rows)      # +-1.09 of the input clips
    x = torch.rand(rows, n, dtype=tdt, device=dev) * 2.2 - 1.1
    y = torch.empty_like(x)
    codes = torch.empty((rows // k, k * n), dtype=torch.int16, device=dev)
    codes2 = torch.empty_like(codes)
    counts = torch.empty((rows, 3), dtype=torch.int64, device=dev) if with_counts else None
    counts2 = torch.empty((rows, 3), dtype=torch.int64, device=dev) if with_counts else None
    fu = distortion.MixDacStage(m, n, gain, mix_offset=mix_offset, dac_offset=dac_offset, interleave=k, dtype=dtype)
    mix = distortion.MixStage(m, n, offset=mix_offset, dtype=dtype)
    dac = distortion.DacStage(gain, n, offset=dac_offset, interleave=k, dtype=dtype, batch=rows)

    def fused():
        fu.apply_torch(x, codes, counts)

    def two():
        mix.apply_torch(x, y)
        dac.apply_torch(y, codes2, counts2)

    def dac_alone():
        dac.apply_torch(y, codes2, counts2)

    fused()
    two()
    torch.cuda.synchronize()
    equal = bool(torch.equal(codes, codes2)) and (counts is None or bool(torch.equal(counts, counts2)))
    t = {name: [] for name in ('fused', 'two', 'dac')}
    for _ in range(2):
        for name, fn in (('fused', fused), ('two', two), ('dac', dac_alone)):
            t[name].append(block(fn, reps))
    ms = {name: round(min(v), 4) for name, v in t.items()}
    spread = {name: round(abs(v[0] - v[1]), 4) for name, v in t.items()}
    es = np.dtype(dtype).itemsize
    model_bytes = fu.reads * n * es + 2 * rows * n
    r = dict(case=case, dtype=kind, rows=rows, n=n, interleave=k, counts=with_counts, reads=int(fu.reads),
             mix_rows_reads=int(mix.reads), kernel=fu.kernel_name(with_counts), equal_to_two_launches=equal,
             fused_ms=ms['fused'], two_ms=ms['two'], dac_ms=ms['dac'], fused_spread_ms=spread['fused'],
             two_spread_ms=spread['two'], dac_spread_ms=spread['dac'], model_bytes=model_bytes,
             fused_GBps=round(model_bytes / ms['fused'] / 1e6, 1), two_over_fused=round(ms['two'] / ms['fused'], 3),
             clipped=None if counts is None else int(counts[:, :2].sum()))
    for st in (fu, mix, dac):
        st.close()
    del x, y, codes, codes2
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='iq,tri,band4,dense')
    ap.add_argument('--dtypes', default='f64,f32')
    ap.add_argument('--shapes', default='256x1000000,2048x100000')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for case in a.cases.split(','):
        shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
        legs = [(kind, rows, n, c) for rows, n in shapes for kind in a.dtypes.split(',') for c in (False, True)]
        if case == 'dense':                               # not the stage's shape: one line
            legs = [('f64', 256, 100000, False)]
        for kind, rows, n, c in legs:
            r = run_leg(case, kind, rows, n, c, a.reps)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
