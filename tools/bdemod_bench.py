#!/usr/bin/env python3
"""IQ trajectories per time bin (waveforms_amd.utils.BinnedDemodulator) on the cases B1-B5, timed with device events.

    python tools/bdemod_bench.py [--cases B1,B4] [--reps 20] [--no-baseline] [--json out.json]

One line per case and trace dtype: ms per apply (median of --reps after a warm-up), `frac` = the input plus the output
bytes, once, over HBM's 8 TB/s, over the time, and on the same traces in the same process
  demod_ms   (a) `Demodulator` with the same tones: the same FMAs without the bin stores -- the floor
  bmm_ms     (b) torch.bmm over x.view(S, W, bin).transpose(0, 1), widened to float64, and e.view(W, bin, 2 nf)
             (the widening is part of the line for int16 and float32 traces; a case whose start or length does not
             let the traces be viewed takes a slice, a copy, first -- also part of the line)
  copy_ms    a device copy of as many bytes as the output has, and the rate it gives: what the extra output bytes
             cost at the copy rate of this process
  allowed_ms demod_ms + the output bytes at that copy rate (the expectation is ours <= this, up to the run-to-run
             spread of two processes)
The trajectories are checked against the bmm line before anything is timed (1e-9 of SUM |x| |e| per bin)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd.utils import BinnedDemodulator, Demodulator, getFTMatrix  # noqa: E402

HBM = 8e12
CASES = {   # name: (shots, N, dtypes, nf, bin, W, start)
    'B1': (65536, 4096, ('i16', ), 8, 128, 32, 0),
    'B2': (65536, 4096, ('i16', 'f32', 'f64'), 8, 128, 32, 0),
    'B3': (65536, 4096, ('i16', 'f32', 'f64'), 8, 16, 256, 0),
    'B4': (65536, 4096, ('f64', ), 8, 100, 40, 3),
    'B5': (1024, 262144, ('i16', ), 4, 4096, 64, 0),
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
    S, N, _, nf, bin, W, start = CASES[name]
    dtype = np.dtype(DTYPES[kind])
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    if kind == 'i16':
        x = torch.randint(-32768, 32768, (S, N), dtype=torch.int16, device=dev)
    else:
        x = torch.randn(S, N, dtype=TORCH[kind], device=dev)
    f = np.linspace(-400e6, 400e6, nf)
    bd = BinnedDemodulator(f, N, bin, start=start, bins=W, dtype=dtype)
    out = torch.empty((S, W, nf), dtype=torch.complex128, device=dev)
    bd.apply_torch(x, out)
    # (b) as one batched real product: (W, S, bin) @ (W, bin, 2 nf)
    used = slice(start, start + W * bin)
    eb = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(bd.e[used])).to(dev)).reshape(W, bin, 2 * nf)

    def bmm():
        xs = x if start == 0 and W * bin == N else x[:, used]
        return torch.bmm(xs.reshape(S, W, bin).transpose(0, 1).to(torch.float64), eb)

    r = dict(case=name, S=S, N=N, nf=nf, bin=bin, W=W, start=start, dtype=dtype.name, kernel=bd.kernel_name(S))
    want = None
    try:
        want = torch.view_as_complex(bmm().reshape(W, S, nf, 2)).transpose(0, 1)
        mag = torch.bmm(x[:, used].reshape(S, W, bin).transpose(0, 1).to(torch.float64).abs(),
                        torch.from_numpy(np.abs(bd.e[used])).to(dev).reshape(W, bin, nf)).transpose(0, 1)
        if not bool(((out - want).abs() <= 1e-9 * mag).all()):
            raise SystemExit(f'{name} {kind}: the trajectories differ from the torch line')
        del want, mag
    except RuntimeError as ex:          # out of memory for the widened copy
        r['check'] = 'skipped: %s' % str(ex).splitlines()[0][:80]
    torch.cuda.empty_cache()
    ms = timed(lambda: bd.apply_torch(x, out), reps)
    bytes_in, bytes_out = S * W * bin * dtype.itemsize, S * W * nf * 16
    roof = (bytes_in + bytes_out) / HBM * 1e3
    r.update(ms=round(ms, 4), roof_ms=round(roof, 4), frac=round(roof / ms, 3))
    if baseline:
        dm = Demodulator(f, N, dtype=dtype)
        iq = torch.empty((S, nf), dtype=torch.complex128, device=dev)
        t_dm = timed(lambda: dm.apply_torch(x, iq), reps)
        src = torch.empty(bytes_out, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        t_copy = timed(lambda: dst.copy_(src), reps)
        del src, dst
        rate = bytes_out / (t_copy * 1e-3)
        allowed = t_dm + bytes_out / rate * 1e3
        r.update(demod_ms=round(t_dm, 4), demod_kernel=dm.kernel_name(S), copy_ms=round(t_copy, 4),
                 copy_TBps=round(rate / 1e12, 3), allowed_ms=round(allowed, 4), ours_over_allowed=round(ms / allowed, 3))
        dm.close()
        try:
            t_bmm = timed(bmm, reps)
            r.update(bmm_ms=round(t_bmm, 4), bmm_over_ours=round(t_bmm / ms, 2))
        except RuntimeError as ex:
            r['bmm'] = 'failed: %s' % str(ex).splitlines()[0][:80]
    bd.close()
    del x, out, eb
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='B1,B2,B3,B4,B5')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--json')
    a = ap.parse_args()
    res, seen = [], set()
    for name in a.cases.split(','):
        for kind in CASES[name][2]:
            key = CASES[name][:2] + (kind, ) + CASES[name][3:]
            if key in seen:                 # B1 is the int16 line of B2
                continue
            seen.add(key)
            r = run_case(name, kind, a.reps, not a.no_baseline)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
