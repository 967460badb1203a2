#!/usr/bin/env python3
"""The segment library (distortion.SegmentLibrary, csrc/wfk_segment_library.hip) timed with device events behind the
segment stage that feeds it, in the same process on the same tensors, next to what a user would do today: download the
packed codes of every pulse and deduplicate them on the host with a dict over byte strings, row by row.

    python tools/segment_library_bench.py [--cases M1,M2,M3] [--widths 1,2] [--shapes 1,16,0] [--reps 10]
                                          [--host-rows 8] [--json out.json]

Cases: M1 = 2048 x 1e5, M2 = 256 x 1e6, M3 = 8 x 1e7 rows of samples, align 16.  A row is a train of gates of 256
samples, one per 1280 samples (20 % duty), each on the same granule phase; a gate's codes are one of D shapes drawn at
random (--shapes; 0: every gate its own codes), the marker in bit 0.  The stage is built with max_segments = the gates
of a row.  One process per case.  One line per case, width and D: ms per library apply and per sizing pass (median,
min and max of --reps event-timed runs after 2 warm-ups), ms per apply of the segment stage in front of it, the
library's download against the stage's download of the packed codes (wall clock, both ending on the host), and the
host composition -- download, then the dict -- on `host_rows` rows scaled to all of them.  The four launches separately
come from a run of this tool under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {'M1': (2048, 10**5), 'M2': (256, 10**6), 'M3': (8, 10**7)}   # name: (rows, n)
GATE, PERIOD, PHASE, ALIGN = 256, 1280, 512, 16


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


def wall(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(float(np.median(ts)), 3), min=round(float(min(ts)), 3), max=round(float(max(ts)), 3))


def host_library(table_r, packed_r, k):
    """the dict over (length, bytes) a host would run on one downloaded row -> (unique, lib_kept)"""
    seen, kept = {}, 0
    for _, length, offset in table_r.tolist():
        key = (length, packed_r[k * offset:k * (offset + length)].tobytes())
        if key not in seen:
            seen[key] = kept
            kept += length
    return len(seen), kept


def run_case(case, widths, shape_counts, reps, host_rows):
    import torch
    from waveforms_amd import distortion
    rows, n = CASES[case]
    dev = torch.device('cuda', 0)
    gates = n // PERIOD
    res = []
    for k in widths:
        st = distortion.SegmentStage(n, rows, k, ALIGN, max_segments=gates)
        lib = distortion.SegmentLibrary.of(st)
        table = torch.empty((rows, gates, 3), dtype=torch.int32, device=dev)
        packed = torch.empty((rows, k * n), dtype=torch.int16, device=dev)
        used = torch.empty((rows, 2), dtype=torch.int64, device=dev)
        plays = torch.empty((rows, gates, 3), dtype=torch.int32, device=dev)
        slots = torch.empty((rows, gates), dtype=torch.int32, device=dev)
        library = torch.empty((rows, k * n), dtype=torch.int16, device=dev)
        lib_used = torch.empty((rows, 2), dtype=torch.int64, device=dev)
        for D in shape_counts:
            g = torch.Generator(device=dev).manual_seed(100 * k + D)
            codes = torch.zeros((rows, k * n), dtype=torch.int16, device=dev)
            body = codes[:, :k * gates * PERIOD].view(rows, gates, k * PERIOD)
            if D:
                shapes = torch.randint(-32768, 32768, (D, k * GATE), dtype=torch.int16, device=dev, generator=g) | 1
                body[:, :, k * PHASE:k * (PHASE + GATE)] = shapes[torch.randint(0, D, (rows, gates), device=dev, generator=g)]
            else:
                body[:, :, k * PHASE:k * (PHASE + GATE)] = torch.randint(
                    -32768, 32768, (rows, gates, k * GATE), dtype=torch.int16, device=dev, generator=g) | 1
            del body
            t_stage = timed(lambda: st.apply_torch(codes, bit=0, table=table, packed=packed, used=used), reps)
            t_lib = timed(lambda: lib.apply_torch(table, packed, used, plays=plays, slots=slots, library=library,
                                                  lib_used=lib_used), reps)
            t_size = timed(lambda: lib.measure_torch(table, packed, used, lib_used=lib_used), reps)
            lib.apply_torch(table, packed, used, plays=plays, slots=slots, library=library, lib_used=lib_used)
            u, lu = used.cpu().numpy(), lib_used.cpu().numpy()
            line = dict(case=case, rows=rows, n=n, width=k, align=ALIGN, shapes=D or 'distinct', gates_per_row=gates,
                        kernels=[lib.kernel_name(i) for i in range(4)], stage_ms=t_stage, library_ms=t_lib,
                        sizing_ms=t_size, library_over_stage=round(t_lib['median'] / t_stage['median'], 2),
                        segments=int(u[:, 0].sum()), kept=int(u[:, 1].sum()), unique=int(lu[:, 0].sum()),
                        lib_kept=int(lu[:, 1].sum()), kept_codes_GBps=round(int(u[:, 1].sum()) * k * 2 / t_lib['median'] / 1e6, 1))
            packed_dl = wall(lambda: st.download(table, packed, used), 5)
            library_dl = wall(lambda: lib.download(plays, slots, library, lib_used, used), 5)
            line.update(packed_download_ms=packed_dl, library_download_ms=library_dl,
                        library_over_packed_download=round(library_dl['median'] / packed_dl['median'], 3))
            hr = min(rows, host_rows)
            down = st.download(table, packed, used)
            t0 = time.perf_counter()
            host = [host_library(down[r][0], down[r][1], k) for r in range(hr)]
            host_ms = (time.perf_counter() - t0) * 1e3 * rows / hr
            differ = sum(int(host[r] != tuple(lu[r].tolist())) for r in range(hr))
            line.update(host_rows=hr, host_dict_ms_scaled=round(host_ms, 2), differ_from_host=differ,
                        host_over_library=round((packed_dl['median'] + host_ms) / (t_lib['median'] + library_dl['median']), 1))
            res.append(line)
            print(json.dumps(line), flush=True)
            del codes
        st.close()
        lib.close()
        del table, packed, used, plays, slots, library, lib_used
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='M1,M2,M3')
    ap.add_argument('--widths', default='1,2')
    ap.add_argument('--shapes', default='1,16,0', help='D shapes the gates are drawn from; 0: all distinct')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-rows', type=int, default=8)
    ap.add_argument('--json')
    ap.add_argument('--child', action='store_true', help='run the one case given in this process')
    a = ap.parse_args()
    cases = a.cases.split(',')
    if a.child or len(cases) == 1:
        res = run_case(cases[0], [int(v) for v in a.widths.split(',')], [int(v) for v in a.shapes.split(',')], a.reps,
                       a.host_rows)
    else:                                                   # one process per case; this one never opens the device
        res = []
        for case in cases:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--cases', case, '--widths', a.widths,
                   '--shapes', a.shapes, '--reps', str(a.reps), '--host-rows', str(a.host_rows)]
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
