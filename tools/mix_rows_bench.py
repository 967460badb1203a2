#!/usr/bin/env python3
"""The mix stage (distortion.MixStage, csrc/wfk_mix_rows.hip) timed with device events, next to two yardsticks on the
same box and the very same tensors in the same process:

  * `out.copy_(x)`, a plain copy of the rows: the stream ceiling (it moves 2 * sizeof(sample) per sample);
  * `torch.matmul(M, x)` with M dense: the alternative a user has today (a GEMM over every zero of M, not
    bit-reproducible against NumPy, NaN * 0 = NaN).

    python tools/mix_rows_bench.py [--cases iq,tri,band4,dense] [--dtypes f64,f32] [--rows 256] [--n 1000000]
                                   [--reps 20] [--json out.json]

Cases on rows x n samples (256 x 1e6 unless given; the output stays resident): iq = 2 x 2 blocks, tri = tridiagonal,
band4 = a band of half-width 4, dense = rows x rows.  One line per case and dtype: ms per apply, per copy and per matmul
(median, min and max of --reps event-timed runs after a warm-up; the three are timed alternately, two blocks of each),
the bytes the stage moves by its traffic model -- (.reads + rows_out) * n * sizeof(sample) -- and its GB/s on them, the
copy's GB/s, the ratio of the two rates, and the largest difference from the matmul on a few rows (the matmul sums in
another order: a few ulps, not zero).
"""
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
    if case == 'iq':
        m = np.zeros((rows, rows))
        for p in range(rows // 2):
            m[2 * p:2 * p + 2, 2 * p:2 * p + 2] = np.eye(2) + 0.05 * rng.standard_normal((2, 2))
        return m
    if case == 'tri':
        return band(rows, 1, rng)
    if case == 'band4':
        return band(rows, 4, rng)
    if case == 'dense':
        return rng.uniform(0.1, 1.0, (rows, rows)) / rows
    raise SystemExit(f'unknown case {case}')


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


def run_leg(case, kind, rows, n, reps):
    dtype = np.float64 if kind == 'f64' else np.float32
    tdt = torch.float64 if kind == 'f64' else torch.float32
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    m = matrix_of(case, rows, rng)
    offset = rng.uniform(-0.01, 0.01, rows)
    x = torch.rand(rows, n, dtype=tdt, device=dev) * 2 - 1
    out = torch.empty_like(x)
    st = distortion.MixStage(m, n, offset=offset, dtype=dtype)
    md = torch.from_numpy(m).to(dev).to(tdt)

    def stage():
        st.apply_torch(x, out)

    def copy():
        out.copy_(x)

    prod = torch.empty_like(x)

    def matmul():
        torch.matmul(md, x, out=prod)

    t = {name: [] for name in ('stage', 'copy', 'matmul')}
    for _ in range(2):
        for name, fn in (('stage', stage), ('copy', copy), ('matmul', matmul)):
            t[name].append(timed(fn, reps))
    stage()
    matmul()
    pick = torch.from_numpy(np.unique(np.r_[0, rows - 1, rng.integers(0, rows, 2)])).to(dev)
    diff = float((out[pick] - (prod[pick] + torch.from_numpy(offset).to(dev).to(tdt)[pick, None])).abs().max())
    ms, cp, mm = (min(b['median'] for b in t[name]) for name in ('stage', 'copy', 'matmul'))
    es = np.dtype(dtype).itemsize
    model_bytes, copy_bytes = (st.reads + st.rows_out) * n * es, 2 * rows * n * es
    r = dict(case=case, dtype=kind, rows=rows, n=n, nnz=int(st.nnz), reads=int(st.reads), kernel=st.kernel_name(),
             stage_ms=t['stage'], copy_ms=t['copy'], matmul_ms=t['matmul'], model_bytes=model_bytes,
             stage_GBps=round(model_bytes / ms / 1e6, 1), copy_GBps=round(copy_bytes / cp / 1e6, 1),
             stage_rate_over_copy_rate=round(model_bytes / ms / (copy_bytes / cp), 4),
             stage_over_copy=round(ms / cp, 4), matmul_over_stage=round(mm / ms, 2),
             stage_GFLOPs=round(2 * st.nnz * n / ms / 1e6, 1), max_abs_diff_from_matmul=diff)
    st.close()
    del x, out, prod, md
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='iq,tri,band4,dense')
    ap.add_argument('--dtypes', default='f64,f32')
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--n', type=int, default=10**6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for case in a.cases.split(','):
        for kind in a.dtypes.split(','):
            r = run_leg(case, kind, a.rows, a.n, a.reps)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
