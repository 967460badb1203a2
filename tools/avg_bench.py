#!/usr/bin/env python3
"""Per-step shot sums (waveforms_amd.utils.TraceAverager) on the cases A1-A3, timed with device events.

    python tools/avg_bench.py [--cases A1,A3] [--dtypes i16,f32,f64] [--reps 20] [--no-baseline] [--json out.json]

One line per case and trace dtype: ms per apply (median of --reps after a warm-up) for the sum alone and for the sum
with the sum of squares, the fraction of the roof (the input bytes, read once, over HBM's 8 TB/s), and on the same
traces in the same process
  torch_sum_ms     traces.view(S // G, G, N).sum(0, dtype=int64 | float64)
  torch_sumsq_ms   that plus the same sum over the widened squares
  copy_ms          a plain device copy of the input bytes (it reads AND writes them: the bandwidth yardstick)
with the ratios torch / ours and copy / ours (above 1: the averager is the faster one).  The sums are checked against
the torch line before anything is timed: bit for bit for int16, to 1e-9 of SUM|x| for floats.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd.utils import TraceAverager  # noqa: E402

HBM = 8e12
CASES = {   # name: (shots, N, steps)
    'A1': (65536, 4096, 1),
    'A2': (65536, 4096, 64),
    'A3': (1024, 262144, 1),
}
DTYPES = {'i16': np.int16, 'f32': np.float32, 'f64': np.float64}
TORCH = {'i16': torch.int16, 'f32': torch.float32, 'f64': torch.float64}


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


def run_case(name, kind, reps, baseline):
    S, N, G = CASES[name]
    dtype = np.dtype(DTYPES[kind])
    wide = torch.int64 if kind == 'i16' else torch.float64
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    if kind == 'i16':
        x = torch.randint(-32768, 32768, (S, N), dtype=torch.int16, device=dev)
    else:
        x = torch.randn(S, N, dtype=TORCH[kind], device=dev)
    av = TraceAverager(N, steps=G, dtype=dtype)
    total, total_sq = (torch.empty((G, N), dtype=wide, device=dev) for _ in range(2))
    av.apply_torch(x, total, total_sq)
    want = x.view(S // G, G, N).sum(0, dtype=wide)
    if kind == 'i16':
        exact = bool((total == want).all())
    else:
        exact = bool(((total - want).abs() <= 1e-9 * x.view(S // G, G, N).abs().sum(0, dtype=wide)).all())
    del want
    if not exact:
        raise SystemExit(f'{name} {kind}: the sums differ from the torch line')
    ms_sum = timed(lambda: av.plan.apply(x.data_ptr(), S, N, 0, total.data_ptr(), N, None, 0, False,
                                         torch.cuda.current_stream().cuda_stream), reps)
    ms_sq = timed(lambda: av.apply_torch(x, total, total_sq), reps)
    bytes_in = S * N * dtype.itemsize
    roof = bytes_in / HBM * 1e3
    r = dict(case=name, S=S, N=N, G=G, dtype=dtype.name, splits=av.splits(S), kernel=av.kernel_name(S),
             sum_ms=round(ms_sum, 4), sumsq_ms=round(ms_sq, 4), roof_ms=round(roof, 4),
             sum_frac_of_roof=round(roof / ms_sum, 3), sumsq_frac_of_roof=round(roof / ms_sq, 3))
    if baseline:
        xv = x.view(S // G, G, N)
        try:
            t_sum = timed(lambda: xv.sum(0, dtype=wide), reps)
            t_sq = timed(lambda: (xv.sum(0, dtype=wide), xv.to(wide).square_().sum(0)), reps)
            dst = torch.empty_like(x)
            t_copy = timed(lambda: dst.copy_(x), reps)
            del dst
            r.update(torch_sum_ms=round(t_sum, 4), torch_sumsq_ms=round(t_sq, 4), copy_ms=round(t_copy, 4),
                     torch_over_sum=round(t_sum / ms_sum, 2), torch_over_sumsq=round(t_sq / ms_sq, 2),
                     copy_over_sum=round(t_copy / ms_sum, 2), copy_over_sumsq=round(t_copy / ms_sq, 2))
        except RuntimeError as ex:          # out of memory for the widened copy
            r['torch_baseline'] = 'failed: %s' % str(ex).splitlines()[0][:80]
    av.close()
    del x, total, total_sq
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='A1,A2,A3')
    ap.add_argument('--dtypes', default='i16,f32,f64')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for name in a.cases.split(','):
        for kind in a.dtypes.split(','):
            r = run_case(name, kind, a.reps, not a.no_baseline)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
