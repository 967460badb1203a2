#!/usr/bin/env python3
"""The segment stage (distortion.SegmentStage, csrc/wfk_segment_rows.hip) timed with device events, next to the torch
composition a user would write today, on the same tensors in the same process -- per row, since its sizes depend on
the data:

    g = pad(m, ...).view(Q, A).any(1);  e = diff(g, prepend=0, append=0)
    q0, q1 = nonzero(e == 1), nonzero(e == -1)            each a synchronisation
    start = q0 A;  length = clamp(q1 A, max=n) - start;  offset = cumsum(length) - length
    packed = masked_select(codes_row, g.repeat_interleave(A)[:n].repeat_interleave(k))

and next to the pinned device-to-host copy of the full code rows, against `download` of what the stage kept.

    python tools/segment_rows_bench.py [--cases M1,M2,M3] [--widths 1,2] [--duties 0,20,100] [--forms bit,marks]
                                       [--align 16] [--reps 10] [--no-chain] [--no-copy] [--json out.json]

Cases: M1 = 2048 x 1e5, M2 = 256 x 1e6, M3 = 8 x 1e7 rows of samples (O1 = 2048 x 100003, not in the default list: rows
that are not 16-byte aligned and take the element paths); gates of 256 samples at the duty given.  One
process per case.  One line per case, width, duty and form: ms per apply and per sizing pass (median, min and max of
--reps event-timed runs after 2 warm-ups) and GB/s against the bytes the form must move -- the codes read twice, the
marks read twice, the kept codes written; the composition on `chain_rows` rows scaled to all of them
(`chain_over_stage`); the full copy and `download` in wall-clock ms, both ending on the host.  The three launches
separately come from a run of this tool under `rocprofv3 --kernel-trace --stats` (tools/collect_profiles.sh segment).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {'M1': (2048, 10**5), 'M2': (256, 10**6), 'M3': (8, 10**7),   # name: (rows, n)
         'O1': (2048, 10**5 + 3)}                                     # odd rows: most are not 16-byte aligned
BIT = 0
GATE = 256
CHAIN_ROWS = 32    # the composition is timed on this many rows at most


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


def composition(codes_row, m_row, k, align):
    import torch
    import torch.nn.functional as F
    n = m_row.numel()
    q = -(-n // align)
    g = F.pad(m_row, (0, q * align - n)).view(q, align).any(1)
    zero = torch.zeros(1, dtype=torch.int8, device=g.device)
    e = torch.diff(g.to(torch.int8), prepend=zero, append=zero)
    q0, q1 = torch.nonzero(e == 1)[:, 0], torch.nonzero(e == -1)[:, 0]
    start = q0 * align
    length = torch.clamp(q1 * align, max=n) - start
    offset = torch.cumsum(length, 0) - length
    keep = g.repeat_interleave(align)[:n].repeat_interleave(k)
    return torch.stack([start, length, offset], 1).to(torch.int32), torch.masked_select(codes_row, keep)


def run_case(case, widths, duties, forms, align, reps, chain, copy):
    import torch
    from waveforms_amd import distortion
    rows, n = CASES[case]
    dev = torch.device('cuda', 0)
    res = []
    for k in widths:
        st = distortion.SegmentStage(n, rows, k, align)
        table = torch.empty((rows, st.max_segments, 3), dtype=torch.int32, device=dev)
        packed = torch.empty((rows, k * n), dtype=torch.int16, device=dev)
        used = torch.empty((rows, 2), dtype=torch.int64, device=dev)
        pinned = torch.empty((rows, k * n), dtype=torch.int16).pin_memory() if copy else None
        for duty in duties:
            g = torch.Generator(device=dev).manual_seed(duty)
            on = torch.rand(rows, (n + GATE - 1) // GATE, device=dev, generator=g) < duty / 100.0
            m = on.repeat_interleave(GATE, dim=1)[:, :n]
            codes = torch.randint(-32768, 32768, (rows, k * n), dtype=torch.int16, device=dev, generator=g)
            codes = (codes & ~(1 << BIT)) | (m.repeat_interleave(k, dim=1).to(torch.int16) << BIT)
            marks = m.to(torch.uint8)
            del on
            for form in forms:
                kw = dict(bit=BIT) if form == 'bit' else dict(marks=marks)
                t = timed(lambda: st.apply_torch(codes, table=table, packed=packed, used=used, **kw), reps)
                ts = timed(lambda: st.measure_torch(codes, used=used, **kw), reps)
                st.apply_torch(codes, table=table, packed=packed, used=used, **kw)
                u = used.cpu().numpy()
                kept = int(u[:, 1].sum())
                moved = 2 * rows * k * n * 2 + (2 * rows * n if form == 'marks' else 0) + kept * k * 2
                line = dict(case=case, rows=rows, n=n, width=k, align=align, duty=duty, form=form,
                            kernels=[st.kernel_name(i, form == 'marks') for i in range(3)], stage_ms=t, sizing_ms=ts,
                            segments=int(u[:, 0].sum()), kept=kept, kept_fraction=round(kept / (rows * n), 4),
                            moved_bytes=moved, stage_GBps=round(moved / t['median'] / 1e6, 1))
                if chain:
                    chain_rows = min(rows, CHAIN_ROWS)

                    def torch_rows():
                        for r in range(chain_rows):
                            composition(codes[r], m[r], k, align)

                    tc = timed(torch_rows, 3, warm=1)
                    differ = 0
                    for r in sorted({0, rows // 2, rows - 1}):
                        want_t, want_p = composition(codes[r], m[r], k, align)
                        c, q = int(u[r, 0]), k * int(u[r, 1])
                        differ += int(c != len(want_t)) + int(q != len(want_p))
                        differ += int((table[r, :c] != want_t).sum()) + int((packed[r, :q] != want_p).sum())
                    line.update(chain_ms=tc, chain_rows=chain_rows, differ_from_chain=differ,
                                chain_over_stage=round(tc['median'] * rows / chain_rows / t['median'], 1))
                if copy:
                    line.update(full_copy_ms=wall(lambda: pinned.copy_(codes, non_blocking=True), 5),
                                download_ms=wall(lambda: st.download(table, packed, used), 5),
                                apply_and_download_ms=wall(lambda: st.download(*st.apply_torch(
                                    codes, table=table, packed=packed, used=used, **kw)), 5))
                res.append(line)
                print(json.dumps(line), flush=True)
            del codes, marks, m
        st.close()
        del table, packed, used, pinned
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='M1,M2,M3')
    ap.add_argument('--widths', default='1,2')
    ap.add_argument('--duties', default='0,20,100')
    ap.add_argument('--forms', default='bit,marks')
    ap.add_argument('--align', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-chain', action='store_true')
    ap.add_argument('--no-copy', action='store_true')
    ap.add_argument('--json')
    ap.add_argument('--child', action='store_true', help='run the one case given in this process')
    a = ap.parse_args()
    cases = a.cases.split(',')
    if a.child or len(cases) == 1:
        res = run_case(cases[0], [int(v) for v in a.widths.split(',')], [int(v) for v in a.duties.split(',')],
                       a.forms.split(','), a.align, a.reps, not a.no_chain, not a.no_copy)
    else:                                                   # one process per case; this one never opens the device
        res = []
        for case in cases:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--cases', case, '--widths', a.widths,
                   '--duties', a.duties, '--forms', a.forms, '--align', str(a.align), '--reps', str(a.reps)]
            cmd += ['--no-chain'] * a.no_chain + ['--no-copy'] * a.no_copy
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
