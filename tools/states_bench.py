#!/usr/bin/env python3
"""IQ points to states and per-step counts (waveforms_amd.utils.StateDiscriminator) on the cases S1-S3, timed with
device events.

    python tools/states_bench.py [--cases S1,S3] [--reps 20] [--no-baseline] [--json out.json]

One line per case: ms per apply (median of --reps after a warm-up), the fraction of the roof (the bytes of the points
read once and of the labels written once, over HBM's 8 TB/s), the kernel and its counter rule, and on the same points
in the same process the torch line

    d = (pts[:, :, None] - c[None]).abs(); lab = d.argmin(-1)
    cnt = torch.nn.functional.one_hot(lab, K).view(R, G, nf, K).sum(0)

as torch_ms with the ratio torch / ours (above 1: the discriminator is the faster one).  The torch line needs a whole
number of cycles, so with S no multiple of the steps it runs on the first (S // G) * G shots, a little less work than
ours.  Before anything is timed the labels are compared with the torch line's (it takes |d| through hypot, so a point
on a bisector may round the other way: the number that differ is printed and must stay below 1e-5 of the points) and
the counts with a bincount of our own labels.  --no-baseline leaves the torch line out altogether (a profile then
shows the discriminator's kernels alone).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveforms_amd.utils import StateDiscriminator  # noqa: E402

HBM = 8e12
CASES = {   # name: (shots, nf, K, steps, joint)
    'S1': (1048576, 8, 2, 1, True),       # the hot-counter case: one step, two states
    'S2': (1048576, 32, 3, 101, False),   # the large-table case: 12 928 counters
    'S3': (65536, 8, 2, 1, True),
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
    return float(np.median(ts))


def run_case(name, reps, baseline):
    S, nf, K, G, with_joint = CASES[name]
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    centres = rng.normal(size=(nf, K)) + 1j * rng.normal(size=(nf, K))
    torch.manual_seed(0)
    state = torch.randint(0, K, (S, nf), device=dev)
    c = torch.from_numpy(centres).to(dev)
    pts = c[torch.arange(nf, device=dev)[None], state] + 0.4 * torch.randn(S, nf, dtype=torch.complex128, device=dev)
    del state
    sd = StateDiscriminator(centres, steps=G)
    labels = torch.empty((S, nf), dtype=torch.uint8, device=dev)
    counts = torch.empty((G, nf, K + 1), dtype=torch.int64, device=dev)
    joint = torch.empty((G, sd.joint_bins), dtype=torch.int64, device=dev) if with_joint else None
    sd.apply_torch(pts, labels, None, counts, joint)
    step = torch.arange(S, device=dev) % G
    flat = ((step[:, None] * nf + torch.arange(nf, device=dev)[None]) * (K + 1) + labels.long()).reshape(-1)
    if not torch.equal(torch.bincount(flat, minlength=counts.numel()).view_as(counts), counts):
        raise SystemExit(f'{name}: the counts differ from a bincount of the labels')
    del step, flat
    R = S // G

    def torch_line():
        d = (pts[:R * G, :, None] - c[None]).abs()
        lab = d.argmin(-1)
        return lab, torch.nn.functional.one_hot(lab, K).view(R, G, nf, K).sum(0)

    differ = None
    if baseline:
        lab_t, cnt_t = torch_line()
        differ = int((lab_t != labels[:R * G]).sum())
        if differ > 1e-5 * S * nf or not torch.equal(cnt_t, counts[:, :, :K]) and differ == 0 and R * G == S:
            raise SystemExit(f'{name}: {differ} labels differ from the torch line, or its counts do')
        del lab_t, cnt_t
    ms = timed(lambda: sd.apply_torch(pts, labels, None, counts, joint), reps)
    ms_labels = timed(lambda: sd.apply_torch(pts, labels), reps)
    roof = S * nf * 17 / HBM * 1e3
    r = dict(case=name, S=S, nf=nf, K=K, steps=G, outputs='labels+counts' + ('+joint' if with_joint else ''),
             kernel=sd.kernel_name(S), ms=round(ms, 4), labels_only_ms=round(ms_labels, 4), roof_ms=round(roof, 4),
             frac_of_roof=round(roof / ms, 3), labels_differing_from_torch=differ)
    if baseline:
        t = timed(torch_line, reps)
        r.update(torch_ms=round(t, 4), torch_over_ours=round(t / ms, 2))
    sd.close()
    del pts, labels, counts, joint
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='S1,S2,S3')
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
