#!/usr/bin/env python3
"""The curve stage (distortion.CurveStage, csrc/wfk_curve_rows.hip) timed with device events, next to the yardstick on
the same box, the very same tensors and the same process: `out.copy_(x)`, a plain copy of the rows -- the stage reads and
writes every sample once, exactly what the copy moves.

    python tools/curve_rows_bench.py [--knots 16,128,1024] [--spacings uniform,log] [--dtypes f64,f32]
                                     [--inputs white,smooth] [--rows 256] [--n 1000000] [--reps 20]
                                     [--variants] [--json out.json] [--md out.md]

One leg per (K, spacing, dtype, input, counts, in place) on rows x n samples (256 x 1e6 unless given; --n 10000000 is
the headline size): ms per apply and per copy (median, min and max of --reps event-timed runs after a warm-up; stage and
copy are timed alternately, two blocks of each), `stage_over_copy` (the ratio of the best medians) and `copy_spread` (the
copy's own run-to-run spread: its larger block median over its smaller one).  Inputs: `white` -- uniform over the knots'
range and 2 % beyond either end, every lane of a wave in another interval; `smooth` -- a train of raised-cosine pulses
over the same range, neighbouring samples in the same or the next interval.  An in-place leg runs on a clone of the
input that is refilled before every timed apply (outside the timed interval) and is compared with the same out-of-place
copy.  --variants adds, for the out-of-place white legs without counts, the plan's experiment switches:
WFK_CURVE_BUCKETS=0 (plain bisection instead of the bucket table) and WFK_CURVE_SPANS=1,2,4,8,16 (the spans a workgroup
walks per copy of its row's tables); the plan's own choice is the leg without a switch."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd import distortion  # noqa: E402


def knots_of(K, spacing):
    rng = np.random.default_rng(K)
    xp = np.linspace(-1.0, 1.0, K) if spacing == 'uniform' else np.geomspace(1e-4, 1.0, K)
    fp = np.cumsum(rng.uniform(0.1, 1.0, K)) / K
    return xp, fp


def input_of(kind, rows, n, lo, hi, tdt, dev):
    if kind == 'white':
        return lo + (hi - lo) * (torch.rand(rows, n, dtype=tdt, device=dev) * 1.04 - 0.02)
    i = torch.arange(n, dtype=torch.float64, device=dev)
    phase = torch.arange(rows, dtype=torch.float64, device=dev)[:, None] * 0.37
    pulse = torch.clamp(torch.sin(i[None, :] * (2 * np.pi / 5000.0) + phase), min=0.0)**2
    return (lo + (hi - lo) * 1.02 * pulse).to(tdt)


def timed(fn, reps, warm=3, before=None):
    """`before` runs ahead of every call of fn, outside the timed interval"""
    for _ in range(warm):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before:
            before()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median=round(float(np.median(ts)), 4), min=round(float(min(ts)), 4), max=round(float(max(ts)), 4))


def run_leg(K, spacing, kind, inp, counts, in_place, x, out, cnt, reps, env=None):
    dtype = np.float64 if kind == 'f64' else np.float32
    rows, n = x.shape
    xp, fp = knots_of(K, spacing)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        st = distortion.CurveStage(xp, fp, n, batch=rows, dtype=dtype)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    work = x.clone() if in_place else x                  # in place the stage runs on a copy that it may overwrite ...
    restore = (lambda: work.copy_(x)) if in_place else None      # ... refilled before every timed apply, outside the interval

    def stage():
        st.apply_torch(work, work if in_place else out, cnt if counts else None)

    def copy():
        out.copy_(x)

    t = {'stage': [], 'copy': []}
    for _ in range(2):
        for name, fn in (('stage', stage), ('copy', copy)):
            t[name].append(timed(fn, reps, before=restore if name == 'stage' else None))
    ms, cp = (min(b['median'] for b in t[name]) for name in ('stage', 'copy'))
    cps = [b['median'] for b in t['copy']]
    nbytes = 2 * rows * n * np.dtype(dtype).itemsize
    r = dict(K=K, spacing=spacing, dtype=kind, input=inp, counts=counts, in_place=in_place, rows=rows, n=n,
             switches=env or {}, spans=int(st.plan.spans), kernel=st.kernel_name(counts), stage_ms=t['stage'],
             copy_ms=t['copy'], stage_GBps=round(nbytes / ms / 1e6, 1), copy_GBps=round(nbytes / cp / 1e6, 1),
             stage_over_copy=round(ms / cp, 4), copy_spread=round(max(cps) / min(cps), 4))
    st.close()
    del work
    return r


def md_table(res):
    lines = ['| K | spacing | dtype | input | counts | in place | switches | spans | stage ms | copy ms | stage GB/s | '
             'copy GB/s | stage_over_copy | copy_spread |', '|' + '---|' * 14]
    for r in res:
        sw = ' '.join(f'{k[10:]}={v}' for k, v in r['switches'].items()) or '-'
        lines.append(f"| {r['K']} | {r['spacing']} | {r['dtype']} | {r['input']} | {int(r['counts'])} | "
                     f"{int(r['in_place'])} | {sw} | {r['spans']} | {min(b['median'] for b in r['stage_ms']):.4f} | "
                     f"{min(b['median'] for b in r['copy_ms']):.4f} | {r['stage_GBps']} | {r['copy_GBps']} | "
                     f"{r['stage_over_copy']:.3f} | {r['copy_spread']:.3f} |")
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--knots', default='16,128,1024')
    ap.add_argument('--spacings', default='uniform,log')
    ap.add_argument('--dtypes', default='f64,f32')
    ap.add_argument('--inputs', default='white,smooth')
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--n', type=int, default=10**6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--variants', action='store_true')
    ap.add_argument('--json')
    ap.add_argument('--md')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    res = []

    def leg(*args, **kw):
        r = run_leg(*args, **kw)
        print(json.dumps(r), flush=True)
        res.append(r)

    for kind in a.dtypes.split(','):
        tdt = torch.float64 if kind == 'f64' else torch.float32
        out = torch.empty(a.rows, a.n, dtype=tdt, device=dev)
        cnt = torch.empty(a.rows, 3, dtype=torch.int64, device=dev)
        for spacing in a.spacings.split(','):
            lo, hi = knots_of(16, spacing)[0][[0, -1]]
            for inp in a.inputs.split(','):
                x = input_of(inp, a.rows, a.n, lo, hi, tdt, dev)
                for K in (int(k) for k in a.knots.split(',')):
                    for counts in (False, True):
                        for in_place in (False, True):
                            leg(K, spacing, kind, inp, counts, in_place, x, out, cnt, a.reps)
                    if a.variants and inp == 'white':
                        leg(K, spacing, kind, inp, False, False, x, out, cnt, a.reps, env={'WFK_CURVE_BUCKETS': '0'})
                        for spans in (1, 2, 4, 8, 16):
                            leg(K, spacing, kind, inp, False, False, x, out, cnt, a.reps,
                                env={'WFK_CURVE_SPANS': str(spans)})
                del x
        del out
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    if a.md:
        with open(a.md, 'w') as f:
            f.write(md_table(res))


if __name__ == '__main__':
    main()
