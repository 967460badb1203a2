#!/usr/bin/env python3
"""Readout demodulation (waveforms_amd.utils.Demodulator) on the roofline cases D1-D5, timed with device events.

    python tools/demod_bench.py [--cases D1,D3] [--reps 20] [--no-baseline] [--json out.json]

One line per case: ms per apply (median of --reps after a warm-up), Gsamples/s, the fraction of the binding
roof (HBM 8 TB/s for bytes = S*N*B_in + S*nf*16 + B read once, fp64 78.6 TFLOP/s for 4*nf*S*N), the max
error against host NumPy on a few rows (relative to |x| @ |e|), and the torch baselines on the same traces:
`traces @ view_as_real(E).reshape(N, 2nf)` (dgemm; f64 only, f32 / i16 traces are first widened) and
`traces.to(complex128) @ E` (zgemm).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd.utils import Demodulator, getFTMatrix  # noqa: E402

HBM, FP64 = 8e12, 78.6e12
CASES = {   # name: (S, N, nf, dtype)
    'D1': (65536, 4096, 8, np.float64),
    'D2': (65536, 4096, 8, np.float32),
    'D3': (65536, 4096, 8, np.int16),
    'D4': (65536, 4096, 32, np.float64),
    'D5': (1, 10**7, 4, np.float64),
}
TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int16): torch.int16}


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


def run_case(name, reps, baseline):
    S, N, nf, dtype = CASES[name]
    dtype = np.dtype(dtype)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    e = getFTMatrix(rng.uniform(-400e6, 400e6, nf), N, rng.uniform(0, 6.3, nf))
    if dtype == np.int16:
        x = torch.randint(-32768, 32768, (S, N), dtype=torch.int16, device=dev)
    else:
        x = torch.randn(S, N, dtype=TORCH[dtype], device=dev)
    dm = Demodulator.from_matrix(e, dtype)
    out = torch.empty(S, nf, dtype=torch.complex128, device=dev)
    ms = timed(lambda: dm.apply_torch(x, out), reps)
    rows = np.unique(np.r_[0, S - 1, rng.integers(0, S, 8)])
    xr = x[torch.from_numpy(rows).to(dev)].cpu().numpy().astype(np.float64)
    err = np.max(np.abs(out[torch.from_numpy(rows).to(dev)].cpu().numpy() - xr @ e) / (np.abs(xr) @ np.abs(e)))
    bytes_ = S * N * dtype.itemsize + S * nf * 16 + N * nf * 16
    flop = 4.0 * nf * S * N
    t_hbm, t_fp = bytes_ / HBM * 1e3, flop / FP64 * 1e3
    roof = max(t_hbm, t_fp)
    r = dict(case=name, S=S, N=N, nf=nf, dtype=dtype.name, kernel=dm.kernel_name(S), ms=round(ms, 4),
             gsamples_s=round(S * N / ms / 1e6, 1), bound='hbm' if t_hbm >= t_fp else 'fp64',
             roof_ms=round(roof, 4), frac_of_roof=round(roof / ms, 3), max_rel_err=float('%.3g' % err))
    if baseline:
        E = torch.from_numpy(e).to(dev)
        Er = torch.view_as_real(E).reshape(N, 2 * nf).contiguous()
        xd = x if dtype == np.float64 else None
        try:
            if xd is not None:
                r['torch_dgemm_ms'] = round(timed(lambda: xd @ Er, reps), 4)
            else:
                r['torch_widen_dgemm_ms'] = round(timed(lambda: x.to(torch.float64) @ Er, reps), 4)
            r['torch_zgemm_ms'] = round(timed(lambda: x.to(torch.complex128) @ E, reps), 4)
        except RuntimeError as ex:          # out of memory for the widened copies of the big cases
            r['torch_baseline'] = 'failed: %s' % str(ex).splitlines()[0][:80]
        torch.cuda.empty_cache()
    dm.close()
    del x, out
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='D1,D2,D3,D4,D5')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--json')
    a = ap.parse_args()
    res = []
    for name in a.cases.split(','):
        r = run_case(name, a.reps, not a.no_baseline)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
