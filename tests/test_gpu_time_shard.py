"""Time-axis sharding ("for a single huge channel optionally time-tile across ranks ... FIR halo of
K - 1 samples each rank can recompute"; reference analogue: chunked sampling with carried IIR state,
waveforms/waveform.py:209-257, FIR crop distortion.py:329-337).  Rank r samples [a_r, b_r) of every row as a
SLICE of the caller's grid (wfk_grid.i0).  Here: every rank of world 2 / 3 emulated in one process on the one
GPU against the unsharded plan, plus the real two-process hand-off of the IIR state over gloo."""
import os
import sys

import numpy as np
import pytest

import cases
import waveforms_amd as wf
from oracle import c_oracle
from waveforms_amd import _engine, _flatten, workloads as wl
from waveforms_amd._dist import TimeShardedFir, TimeShardedIir, TimeShardedSampler, channel_block
from waveforms_amd._sampling import BatchSampler
from waveforms_amd.distortion import SampledFir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(kind):
    if kind == 'lean':      # C2's channel spec on a fine grid: the lean kernel
        return [wl.sum_channel(wf, 100, 1000 + c) for c in range(2)], ('linspace', 0.0, 100 * wl.SPAN, 1_500_007, False)
    if kind == 'short':     # AWG sample rate: the short-piece tier
        return [wl.awg_channel(wf, c, 60000, 2e9) for c in range(2)], wl.awg_grid(60000, 2e9)
    if kind == 'endpoint':  # np.linspace(endpoint=True): the overridden last sample belongs to the last rank only
        return [cases.CASES['readme_x'][0](wf)], ('linspace', -1e-6, 9e-6, 400_001, True)
    # erf edges + sinc: generic terms, the general kernel
    w = (wf.square(40e-9, edge=8e-9) >> 100e-9) * wf.cos(2 * np.pi * 90e6) + 0.1 * wf.sinc(2e8) * (wf.square(300e-9) >> 150e-9)
    return [w], ('linspace', 0.0, 300e-9, 250_003, False)


@pytest.mark.parametrize('kind', ['lean', 'short', 'endpoint', 'generic'])
@pytest.mark.parametrize('world', [2, 3])
def test_time_slices_reproduce_the_whole_plan(kind, world):
    import torch
    chans, grid = _rows(kind)
    whole = BatchSampler(chans, grid)
    ref = whole.to_host(np.float64)
    ora = c_oracle.eval_grid(_flatten.flatten(chans), _flatten.grid_from_desc(grid))
    pk = max(1.0, float(np.abs(ora).max()))       # (README x with DRAGScaling = 0.2 peaks at 2.6e7: peak-relative bounds)
    assert np.max(np.abs(ref - ora)) <= 1e-9 * pk
    got = np.empty_like(ref)
    for rank in range(world):
        ts = TimeShardedSampler(chans, grid, rank, world)
        assert ts.lo == ts.start and ts.hi == ts.stop and ts.n == ts.stop - ts.start
        if kind != 'endpoint':      # (README x has its pulses in the first fifth of the window: a slice of zeros is a fill)
            assert ts.local.plan.kernel_name().split('<')[0] == whole.plan.kernel_name().split('<')[0]     # same tier
        out = torch.full((ts.n_channels, ts.n + 3), 9.0, dtype=torch.float64, device='cuda')
        ts.launch_torch(out)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.all(o[:, ts.n:] == 9.0)
        got[:, ts.start:ts.stop] = o[:, ts.own]
        # integer part: the slice's piece indices are the whole plan's, shifted and clipped
        for m in range(len(chans)):
            assert np.array_equal(ts.local.plan.member_index(m),
                                  np.clip(whole.plan.member_index(m) - ts.lo, 0, ts.hi - ts.lo))
        ts.close()
    assert np.max(np.abs(got - ref)) <= 1e-12 * pk, kind   # (tile / seed alignment differs: rounding only)
    assert np.max(np.abs(got - ora)) <= 1e-9 * pk
    whole.close()


@pytest.mark.parametrize('kind,K', [('lean', 1024), ('short', 1024), ('lean', 33)])
def test_fir_with_recomputed_halo(kind, K):
    import torch
    chans, grid = _rows(kind)
    ker = wl.c4_kernel(K)
    whole = SampledFir(chans, grid, ker)
    ref = whole.to_host()
    whole.close()
    for world in (2, 3):
        got = np.empty_like(ref)
        for rank in range(world):
            tf = TimeShardedFir(chans, grid, ker, rank, world)
            hl, hr = K - 1 - K // 2, K // 2
            assert tf.lo == max(0, tf.start - hl) and tf.hi == min(ref.shape[1], tf.stop + hr)
            out = torch.empty((tf.n_channels, tf.n), dtype=torch.float64, device='cuda')
            tf.launch_torch(out)
            torch.cuda.synchronize()
            got[:, tf.start:tf.stop] = out.cpu().numpy()[:, tf.own]
            tf.close()
        assert np.max(np.abs(got - ref)) <= 1e-12, (kind, K, world)
    # and against the oracle: sampled by the C oracle, filtered by the FIR definition
    y = c_oracle.eval_grid(_flatten.flatten(chans[:1]), _flatten.grid_from_desc(grid))[0]
    assert np.max(np.abs(got[0] - c_oracle.fir(y, ker))) <= 1e-10


def test_iir_state_handed_from_slice_to_slice():
    import torch
    from scipy.signal import butter, sosfilt, sosfilt_zi
    chans, grid = _rows('lean')
    sos = butter(4, 0.02, output='sos')
    secs = [(r[:3], r[3:]) for r in sos]
    y = c_oracle.eval_grid(_flatten.flatten(chans), _flatten.grid_from_desc(grid))
    zi0 = sosfilt_zi(sos) * 0.3
    want = np.stack([sosfilt(sos, row - 0.1, zi=zi0)[0] + 0.1 for row in y])
    for world in (1, 2, 3):
        got = np.empty_like(want)
        state = torch.as_tensor(np.broadcast_to(zi0.reshape(-1), (len(chans), zi0.size)).copy(), device='cuda')
        for rank in range(world):
            ts = TimeShardedSampler(chans, grid, rank, world)
            iir = TimeShardedIir(secs, ts)
            buf = torch.empty((ts.n_channels, ts.n), dtype=torch.float64, device='cuda')
            ts.launch_torch(buf)
            state = iir.apply_local(buf, buf, state, 0.1)          # in place; zf -> the next slice's zi
            torch.cuda.synchronize()
            got[:, ts.start:ts.stop] = buf.cpu().numpy()
            iir.close()
            ts.close()
        assert np.max(np.abs(got - want)) <= 1e-10, world
        zf_want = np.stack([sosfilt(sos, row - 0.1, zi=zi0)[1].reshape(-1) for row in y])
        assert np.max(np.abs(state.cpu().numpy() - zf_want)) <= 1e-10


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from scipy.signal import butter, sosfilt
        torch.cuda.set_device(0)                    # both ranks on the one GPU of the box
        _engine.set_device(0)
        chans, grid = _rows('lean')
        sos = butter(2, 0.05, output='sos')
        ts = TimeShardedSampler(chans, grid, rank, world)
        iir = TimeShardedIir([(r[:3], r[3:]) for r in sos], ts)
        buf = torch.empty((ts.n_channels, ts.n), dtype=torch.float64, device='cuda')
        ts.launch_torch(buf)
        zf = iir.apply_torch(buf, buf, initial=0.0)         # recv <- rank - 1, filter, send -> rank + 1
        torch.cuda.synchronize()
        y = c_oracle.eval_grid(_flatten.flatten(chans), _flatten.grid_from_desc(grid))
        want = np.stack([sosfilt(sos, row) for row in y])
        err = float(np.max(np.abs(buf.cpu().numpy() - want[:, ts.start:ts.stop])))
        assert err <= 1e-10, err
        assert (zf is not None) == (rank == world - 1)
        # result placement in slabs on root's host (time slices gathered as row blocks of a transposed job
        # would be the caller's business; here: the channel-block form on real device tensors)
        from waveforms_amd._dist import gather_rows_to_host
        a, b = channel_block(5, rank, world)
        rows = torch.arange(a, b, dtype=torch.float64, device='cuda')[:, None].repeat(1, 1000)
        host = gather_rows_to_host(rows, 5, root=0, slab_bytes=8000 * 2)
        if rank == 0:
            assert np.array_equal(host[:, 7], np.arange(5.0))
        # BOUNDED device memory on root: 128 rows over 2 ranks in slabs of ONE row = 64 gathers; root may hold its
        # block + the staging slab + the ring of 2 x world receive slabs, whatever the number of gathers
        nrow, ncol = 128, 1 << 17
        a, b = channel_block(nrow, rank, world)
        rows = torch.arange(a, b, dtype=torch.float64, device='cuda')[:, None].repeat(1, ncol)
        slab = ncol * 8
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        host = gather_rows_to_host(rows, nrow, root=0, slab_bytes=slab)
        peak = torch.cuda.max_memory_allocated() - base
        assert peak <= 3 * world * slab + (1 << 20), (peak, slab)
        if rank == 0:
            assert np.array_equal(host[:, 0], np.arange(float(nrow))) and np.array_equal(host[:, -1], np.arange(float(nrow)))
        q.put((rank, 'ok'))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_two_processes_hand_the_iir_state_on():
    """the real hand-off: two rank processes (gloo rendezvous on 127.0.0.1, both on the box's one GPU), rank 1
    waits for rank 0's final state"""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, 'ok'), (1, 'ok')], res


def test_more_ranks_than_samples_and_tiny_slices():
    """edge cases of the time cut: slices of 0 / 1 / 2 samples (world > n), a FIR whose halo is longer than the
    slice, a grid of one sample; every rank emulated in turn against the whole plan"""
    import torch
    w = (wf.gaussian(20e-9) >> 15e-9) * wf.cos(2 * np.pi * 100e6) + 0.25
    ker = wl.c4_kernel(33)
    for n, world in ((5, 8), (1, 3), (40, 7), (300, 4)):
        grid = ('linspace', 0.0, 30e-9, n, False)
        ref = BatchSampler([w], grid).to_host(np.float64)
        fref = SampledFir([w], grid, ker).to_host()
        got, fgot = np.full_like(ref, np.nan), np.full_like(ref, np.nan)
        for rank in range(world):
            ts = TimeShardedSampler([w], grid, rank, world)
            assert ts.n == ts.stop - ts.start
            out = torch.zeros((1, max(ts.n, 1)), dtype=torch.float64, device='cuda')
            ts.launch_torch(out)
            torch.cuda.synchronize()
            got[:, ts.start:ts.stop] = out.cpu().numpy()[:, :ts.n][:, ts.own]
            ts.close()
            tf = TimeShardedFir([w], grid, ker, rank, world)
            if tf.stop > tf.start:
                fo = torch.zeros((1, tf.n), dtype=torch.float64, device='cuda')
                tf.launch_torch(fo)
                torch.cuda.synchronize()
                fgot[:, tf.start:tf.stop] = fo.cpu().numpy()[:, tf.own]
            tf.close()
        assert np.max(np.abs(got - ref)) <= 1e-12, (n, world)
        assert np.max(np.abs(fgot - fref)) <= 1e-12, (n, world)


def _slice_rows(kind):
    """two channels (one with a complex amplitude) whose slice runs the general kernel's build `kind`"""
    if kind == 'fused':       # fused ops only (the lean tier switched off)
        chans = [wl.sum_channel(wf, 6, 1000), (0.4 - 0.7j) * wl.sum_channel(wf, 6, 1001)]
        return chans, ('linspace', 0.0, 6 * wl.SPAN, 50000, False), {'WFK_DISABLE_LEAN': '1'}, ',false,false,false,16>'
    if kind == 'generic':     # two tables in one piece: generic terms, nothing for the direct tier
        hann = lambda m: wf.samplingPoints(-wl.SPAN / 2, wl.SPAN / 2, np.hanning(m))
        w = ((hann(1000) * (wf.cos(2e9) + wf.cos(2.5e9))) >> 40e-9) + (hann(100) >> 44e-9)
        return [w, (0.3 + 0.2j) * w], ('linspace', 0.0, 80e-9, 40000, False), {'WFK_DISABLE_MIXED': '1'}, ',false,true,false,16>'
    return [_rows('generic')[0][0], (1 - 0.5j) * _rows('generic')[0][0]], ('linspace', 0.0, 300e-9, 25003, False), {}, ',false,true,true,16>'


@pytest.mark.parametrize('kind', ['fused', 'generic', 'direct'])
def test_float_and_complex_slices_of_the_general_kernel(kind, monkeypatch):
    """wfk_sample_slice / wfk_sample_wide_slice for every output kind: three tiles of a grid from a sample index that is
    no multiple of the tile, against the NumPy oracle at the slice's own times"""
    from oracle import np_oracle
    chans, grid, env, tail = _slice_rows(kind)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = _flatten.grid_slice(_flatten.grid_from_desc(grid), 5001, 5001 + 3 * 4096 + 37)
    plan = _engine.Plan(_flatten.flatten(chans), grid=g)
    t = _flatten.grid_values(g)
    ref = np.stack([np_oracle.call(w, t) for w in chans])
    pk = max(1.0, float(np.abs(ref).max()))
    for dt, tol in ((np.float64, 1e-9), (np.float32, cases.FP32_TOL), (np.complex128, 1e-9), (np.complex64, cases.FP32_TOL)):
        name = plan.kernel_name(dt)
        assert name.startswith(('wfk_sample<', 'wfk_sample_wide<')) and name.endswith(tail), name
        want = ref if np.dtype(dt).kind == 'c' else ref.real
        err = float(np.max(np.abs(plan.run_host(dt) - want)))
        print(kind, np.dtype(dt).name, name, 'err / peak %.3g' % (err / pk))
        assert err <= tol * pk, (kind, dt, err)
    plan.close()
