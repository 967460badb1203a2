#!/usr/bin/env python3
"""The segment player (distortion.SegmentPlayer, csrc/wfk_segment_play.hip) timed with device events, in the same
process on the same tensors, next to two yardsticks: a plain `copy_` of the same (rows, k n) int16 rows, and the host
path it replaces -- `cpu()` of the dense rows plus `expand_segments` per row.

    python tools/segment_play_bench.py [--cases P1,P2,P3] [--widths 1,2] [--reps 20] [--host-rows 8] [--json out.json]

Cases: P1 = 2048 x 1e5, P2 = 256 x 1e6, P3 = 8 x 1e7 rows of samples.  A row is a train of pulses of 60 samples, one
per 300 (20 % duty), off the granule's phase, the codes of a pulse one of 16 shapes drawn at random, the marker in bit
0; it is cut by a SegmentStage at align 16 and folded by a SegmentLibrary.  Sources: `stage` = the stage's table and
packed codes (offsets multiples of 16); `library` = the library's plays and codes moved one sample up, so that every
lib_offset is odd and no source chunk is aligned.  Modes: play (out alone), verify (expect alone), both.  One process
per case.  One line per case, width, source and mode: ms per apply (median, min and max of --reps event-timed runs
after 2 warm-ups), the bytes the contract moves (2 k n written + 2 k played read, + 2 k n for expect) over 8 TB/s over
that time as `frac`, the `copy_` of the dense rows, and the host path on `host_rows` rows scaled to all of them."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {'P1': (2048, 10**5), 'P2': (256, 10**6), 'P3': (8, 10**7)}   # name: (rows, n)
PULSE, PERIOD, PHASE, ALIGN, SHAPES = 60, 300, 37, 16, 16
PEAK = 8e12                                                           # bytes per second


def timed(fn, reps, warm=2):
    import torch
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


def run_case(case, widths, reps, host_rows):
    import torch
    from waveforms_amd import distortion
    rows, n = CASES[case]
    dev = torch.device('cuda', 0)
    pulses = n // PERIOD
    res = []
    for k in widths:
        g = torch.Generator(device=dev).manual_seed(100 * k)
        codes = torch.zeros((rows, k * n), dtype=torch.int16, device=dev)
        body = codes[:, :k * pulses * PERIOD].view(rows, pulses, k * PERIOD)
        shapes = torch.randint(-32768, 32768, (SHAPES, k * PULSE), dtype=torch.int16, device=dev, generator=g) | 1
        body[:, :, k * PHASE:k * (PHASE + PULSE)] = shapes[torch.randint(0, SHAPES, (rows, pulses), device=dev, generator=g)]
        del body
        st = distortion.SegmentStage(n, rows, k, ALIGN, max_segments=pulses)
        table, packed, used = st.apply_torch(codes, bit=0)
        lib = distortion.SegmentLibrary.of(st)
        plays, _, library, lib_used = lib.apply_torch(table, packed, used)
        assert int(lib_used[:, 1].max()) < n
        odd_plays = plays.clone()
        odd_plays[:, :, 2] += 1                                       # every lib_offset odd: no aligned source chunk
        odd_library = torch.zeros_like(library)
        odd_library[:, k:] = library[:, :-k]
        out = torch.empty((rows, k * n), dtype=torch.int16, device=dev)
        report = torch.empty((rows, 4), dtype=torch.int64, device=dev)
        t_copy = timed(lambda: out.copy_(codes), reps)
        hr = min(rows, host_rows)
        t0 = time.perf_counter()
        dense = codes[:hr].cpu().numpy()
        host_copy_ms = (time.perf_counter() - t0) * 1e3 * rows / hr
        down = st.download(table, packed, used)
        t0 = time.perf_counter()
        host_differ = sum(int(not np.array_equal(distortion.expand_segments(*down[r], n, 0, width=k), dense[r]))
                          for r in range(hr))
        host_expand_ms = (time.perf_counter() - t0) * 1e3 * rows / hr
        for source, (t, y, player) in (('stage', (table, packed, distortion.SegmentPlayer.of(st))),
                                       ('library', (odd_plays, odd_library, distortion.SegmentPlayer.of(lib, n)))):
            modes = (('play', lambda: player.apply_torch(t, y, used, out=out, report=report)),
                     ('verify', lambda: player.verify_torch(t, y, used, codes, report=report)),
                     ('both', lambda: player.apply_torch(t, y, used, out=out, expect=codes, report=report)))
            for mode, fn in modes:
                ms = timed(fn, reps)
                fn()
                r = report.cpu().numpy()
                played = int(r[:, 0].sum())
                moved = 2 * k * ((rows * n if mode != 'verify' else 0) + played + (rows * n if mode != 'play' else 0))
                line = dict(case=case, rows=rows, n=n, width=k, align=ALIGN, source=source, mode=mode,
                            kernels=[player.kernel_name(0), player.kernel_name({'play': 1, 'verify': 2, 'both': 3}[mode])],
                            ms=ms, bytes=moved, frac=round(moved / PEAK / (ms['median'] * 1e-3), 4),
                            copy_ms=t_copy, over_copy=round(ms['median'] / t_copy['median'], 3),
                            segments=int(used[:, 0].sum()), played=played, differ=int(r[:, 1].sum()),
                            stray=int(r[:, 2].sum()), bad_rows=int((r[:, 0] < 0).sum()),
                            out_equals_codes=bool(torch.equal(out, codes)) if mode != 'verify' else None,
                            host_rows=hr, host_cpu_ms_scaled=round(host_copy_ms, 2),
                            host_expand_ms_scaled=round(host_expand_ms, 2), host_differ=host_differ,
                            host_over_player=round((host_copy_ms + host_expand_ms) / ms['median'], 1))
                res.append(line)
                print(json.dumps(line), flush=True)
            player.close()
        st.close()
        lib.close()
        del codes, table, packed, used, plays, library, odd_plays, odd_library, out
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='P1,P2,P3')
    ap.add_argument('--widths', default='1,2')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-rows', type=int, default=8)
    ap.add_argument('--json')
    ap.add_argument('--child', action='store_true', help='run the one case given in this process')
    a = ap.parse_args()
    cases = a.cases.split(',')
    if a.child or len(cases) == 1:
        res = run_case(cases[0], [int(v) for v in a.widths.split(',')], a.reps, a.host_rows)
    else:                                                   # one process per case; this one never opens the device
        res = []
        for case in cases:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--cases', case, '--widths', a.widths,
                   '--reps', str(a.reps), '--host-rows', str(a.host_rows)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            sys.stderr.write(out.stderr)
            if out.returncode:
                sys.exit(f'{case}: exit status {out.returncode}')
            for row in out.stdout.splitlines():
                if row.startswith('{'):
                    print(row, flush=True)
                    res.append(json.loads(row))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
