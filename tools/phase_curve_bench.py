"""Where the time of one `PhaseCurve` evaluation goes (GPU machine only; reads no reference sources).

    python tools/phase_curve_bench.py [--rows 1,9,256,4096] [--reps 5]

The demo shape: 0.1 * (square(2 us) << 1 us) at 2 GS/s (80 000 samples), pulse 10 ns, start 25 ns, 60 probe times,
two time constants per row.  Per row count P, in ms per evaluation of P parameter sets (median of --reps):
  design   host: exp_decay_filter for every section of every row
  build    host: per-row IIR plan (quad-precision block tables, rebuilt for every new parameter set) + upload
  iir      device: the iir_rows_tile launch, every row reading the one sampled wave
  probe    device: the boxprobe_wave launch
  total    pc.rows_torch + synchronise, wall clock
  host     the same P curves by the NumPy / SciPy restatement (lfilter on the combined (b, a), np.convolve,
           np.interp), measured on min(P, 16) rows and scaled
One JSON line per P."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', default='1,9,256,4096')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch

    import phase_curve_ref as ref
    import waveforms_amd as wf
    from waveforms_amd import _engine, distortion

    sr, pw, start = 2e9, 10e-9, 25e-9
    wav = 0.1 * (wf.square(2e-6) << 1e-6)
    t = ref.DEMO_T
    t0 = time.perf_counter()
    pc = distortion.PhaseCurve(t, ref.DF_DPHI, pw, start, wav, sr)
    torch.cuda.synchronize()
    print(json.dumps({'setup_ms': round(1e3 * (time.perf_counter() - t0), 3), 'num': pc.num, 'nq': pc.nq,
                      'device': torch.cuda.get_device_name(0)}))
    x_host = wav(pc.tlist)
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream().cuda_stream
    for P in [int(v) for v in args.rows.split(',')]:
        rows = np.array([-0.03, 0.1e-6, 0.02, 0.3e-6]) * rng.uniform(0.8, 1.2, (P, 4))
        pc.rows_torch(rows)                                   # warm-up: workspace, code objects
        torch.cuda.synchronize()
        rec = {k: [] for k in ('design', 'build', 'iir', 'probe', 'total')}
        for _ in range(args.reps):
            t0 = time.perf_counter()
            secs = [pc.sections(p)[0] for p in rows]
            t1 = time.perf_counter()
            plan = _engine.IirRowsPlan(secs, pc.num, np.float64)
            t2 = time.perf_counter()
            kname = plan.kernel_name()
            ws = pc._ws
            out = torch.empty((P, pc.nq), dtype=torch.float64, device=ws.device)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            plan.apply_shared_in(pc._x.data_ptr(), ws.data_ptr(), ws.stride(0), stream=stream)
            ev[1].record()
            pc.probe.apply(ws.data_ptr(), P, ws.stride(0), out.data_ptr(), pc.nq, stream)
            ev[2].record()
            torch.cuda.synchronize()
            plan.close()
            rec['design'].append(1e3 * (t1 - t0))
            rec['build'].append(1e3 * (t2 - t1))
            rec['iir'].append(ev[0].elapsed_time(ev[1]))
            rec['probe'].append(ev[1].elapsed_time(ev[2]))
            t3 = time.perf_counter()
            pc.rows_torch(rows)
            torch.cuda.synchronize()
            rec['total'].append(1e3 * (time.perf_counter() - t3))
        m = min(P, 16)
        t4 = time.perf_counter()
        for p in rows[:m]:
            ref.restated(t, p, ref.DF_DPHI, pw, start, lambda _t: x_host, sr)
        host = 1e3 * (time.perf_counter() - t4) * P / m
        line = {'P': P, 'kernels': [kname, pc.probe.kernel_name()]}
        line.update({k + '_ms': round(statistics.median(v), 4) for k, v in rec.items()})
        line['host_ms'] = round(host, 3)
        print(json.dumps(line), flush=True)
    pc.close()


if __name__ == '__main__':
    main()
