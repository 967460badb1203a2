#!/usr/bin/env python3
"""The marker stage (distortion.MarkerStage, csrc/wfk_marker_rows.hip) timed with device events, next to the torch
composition a user would write today, on the same box and the very same tensors in the same process:

    a = x.abs() > t                                   (k = 2: a[0::2] | a[1::2])
    m = max_pool1d(pad(a.half(), (trail, lead)), lead + trail + 1, stride=1)         one-sided padding
    codes = (codes & ~(1 << bit)) | (m.short().repeat_interleave(k, 1) << bit)       or m.byte() for the bytes form

(the composition counts nothing; the stage's counts legs are timed against the same composition).

    python tools/marker_rows_bench.py [--cases M1,M2,M3] [--dtypes f64,f32] [--groups 1,2] [--forms bytes,codes]
                                      [--edges 0,32,4096] [--reps 10] [--chain-reps 3] [--json out.json]

Cases (the shapes of tools/shift_rows_bench.py): M1 = 2048 x 1e5, M2 = 256 x 1e6, M3 = 8 x 1e7 input rows; gates of
256 samples at a duty of 20 %, exact zeros between them.  One line per case, dtype, group, form, edge (lead = trail)
and with / without counts: ms per apply (median, min and max of --reps event-timed runs after a warm-up) and GB/s
against the bytes the form must move per marker sample -- k * sizeof(sample) read, and 1 written (bytes) or 2 k read
and 2 k written (codes): float64, k = 1, into codes is 8 + 2 + 2 B.  The composition is timed once per case, dtype,
group, form and edge (--chain-reps runs; where the pooling window is 8193 samples, one run over 64 marker rows,
`chain_rows`, scaled to all rows in `chain_over_stage`), and the two results are compared on a few rows at the size
that is timed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd import distortion  # noqa: E402

CASES = {   # name: (input rows, n)
    'M1': (2048, 10**5),
    'M2': (256, 10**6),
    'M3': (8, 10**7),
}
DTYPES = {'f64': np.float64, 'f32': np.float32}
BIT = 0
CHAIN_ROWS = 64    # the composition runs on this many marker rows at a time at most (its temporaries are large)


def timed(fn, reps, warm=2):
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


def gates(rows, n, tdt, dev):
    """uniform noise inside gates of 256 samples at a duty of 20 %, exact zeros between them"""
    g = torch.Generator(device=dev).manual_seed(0)
    on = torch.rand(rows, (n + 255) // 256, device=dev, generator=g) < 0.2
    x = torch.rand(rows, n, dtype=tdt, device=dev, generator=g) + 0.1
    x *= on.repeat_interleave(256, dim=1)[:, :n]
    return x


def composition(x, k, edge, threshold, codes):
    """the markers of x by torch ops -> uint8 (rows / k, n), or `codes` with BIT replaced (a new tensor)"""
    a = x.abs() > threshold
    if k == 2:
        a = a[0::2] | a[1::2]
    m = F.max_pool1d(F.pad(a.to(torch.float16), (edge, edge)), 2 * edge + 1, stride=1) if edge else a
    if codes is None:
        return m.to(torch.uint8)
    return (codes & ~(1 << BIT)) | (m.to(torch.int16).repeat_interleave(k, dim=1) << BIT)


def run_group(case, kind, k, form, edges, reps, chain_reps):
    rows, n = CASES[case]
    dtype = DTYPES[kind]
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    dev = torch.device('cuda', 0)
    x = gates(rows, n, tdt, dev)
    out_rows = rows // k
    es = np.dtype(dtype).itemsize
    moved = out_rows * n * (k * es + (1 if form == 'bytes' else 4 * k))
    if form == 'codes':
        filled = torch.randint(-32768, 32768, (out_rows, k * n), dtype=torch.int16, device=dev)
        out = filled.clone()
    else:
        filled, out = None, torch.empty((out_rows, n), dtype=torch.uint8, device=dev)
    counts = torch.empty((out_rows, 2), dtype=torch.int64, device=dev)
    res = []
    for edge in edges:
        st = distortion.MarkerStage(n, lead=edge, trail=edge, group=k, dtype=dtype, batch=rows)
        chain_rows = min(out_rows, CHAIN_ROWS)
        slow = edge > 1024                       # a pooling window of thousands of samples: CHAIN_ROWS marker rows only
        timed_rows = chain_rows if slow else out_rows

        def chain():
            for r0 in range(0, timed_rows, chain_rows):
                composition(x[r0 * k:(r0 + chain_rows) * k], k, edge, 0.0,
                            None if filled is None else filled[r0:r0 + chain_rows])

        chain_ms = timed(chain, 1 if slow else chain_reps, warm=0 if slow else 1)
        for with_counts in (False, True):
            c = counts if with_counts else None

            def stage():
                if form == 'codes':
                    st.apply_codes_torch(x, out, BIT, c)
                else:
                    st.apply_torch(x, out, c)

            t = timed(stage, reps)
            # parity with the composition on a few marker rows, at the size that is timed
            if form == 'codes':
                out.copy_(filled)
            stage()
            pick = sorted({0, out_rows - 1, out_rows // 2})
            differ = 0
            for g in pick:
                want = composition(x[g * k:(g + 1) * k], k, edge, 0.0, None if filled is None else filled[g:g + 1])
                differ += int((out[g:g + 1] != want).sum())
            ms = t['median']
            res.append(dict(case=case, dtype=kind, rows=rows, n=n, group=k, form=form, edge=edge, counts=with_counts,
                            kernel=st.kernel_name(codes=form == 'codes', counts=with_counts), stage_ms=t,
                            chain_ms=chain_ms, chain_rows=timed_rows, moved_bytes=moved,
                            stage_GBps=round(moved / ms / 1e6, 1),
                            chain_over_stage=round(chain_ms['median'] * out_rows / timed_rows / ms, 2),
                            differ_from_chain=differ,
                            high_pulses=[int(v) for v in counts.sum(dim=0).cpu()] if with_counts else None))
            print(json.dumps(res[-1]), flush=True)
        st.close()
    del x, out, filled
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='M1,M2,M3')
    ap.add_argument('--dtypes', default='f64,f32')
    ap.add_argument('--groups', default='1,2')
    ap.add_argument('--forms', default='bytes,codes')
    ap.add_argument('--edges', default='0,32,4096')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--chain-reps', type=int, default=3)
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for case in a.cases.split(','):
        for kind in a.dtypes.split(','):
            for k in (int(v) for v in a.groups.split(',')):
                for form in a.forms.split(','):
                    res += run_group(case, kind, k, form, [int(v) for v in a.edges.split(',')], a.reps, a.chain_reps)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
