"""The binned demodulator on the device (utils.BinnedDemodulator, csrc/wfk_bdemod.hip) against the referee
tests/bdemod_ref.py: |device - ref| <= 1e-12 * (|x| @ |e| over the bin) element by element (test_gpu_demod.py's bound,
per bin; written as <=, the bound is 0 where a bin's samples are 0), over trace dtypes, tone counts (column buckets and
blocks), shot counts around the 64-shot block, two record lengths and bins that are one sample, odd, a whole number of
16-byte segments or not, aligned or not, and the whole record; an exact integer case, NaN isolation, row windows and
guards, far rows, determinism, streams, graph replay, the rest of the readout chain and the plain-C consumer.

Every comparison prints its largest |device - ref| as a fraction of the bound (python -m pytest tests/test_gpu_bdemod.py
-s); on an MI355X the largest over the whole file is 3.8e-4 (float32, nf = 9, bin = 16), and 1.5e-5 of the summed bounds
for the bins of a shot against the demodulator."""
import os
import subprocess

import numpy as np
import pytest
import torch

import bdemod_ref as ref
from graph_replay import eager, replay, sentinels_left
from row_windows import FarWindow, Window, bits_equal, free_far_arena
from waveforms_amd import _engine
from waveforms_amd.utils import BinnedDemodulator, Demodulator, StateDiscriminator, classify_points, getFTMatrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda', 0)
TYPE_NAME = {np.dtype(np.float64): 'double', np.dtype(np.float32): 'float', np.dtype(np.int16): 'short'}


@pytest.fixture(scope='module', autouse=True)
def far_arena():
    """the far rows' arena goes back to the device when the module is done"""
    yield
    free_far_arena()


def traces(rng, S, N, dtype):
    if np.dtype(dtype) == np.int16:
        return rng.integers(-32768, 32768, size=(S, N), dtype=np.int16)
    return rng.normal(size=(S, N)).astype(dtype)


def tones(rng, nf, N, bin):
    return getFTMatrix(rng.uniform(-400e6, 400e6, nf), N, rng.uniform(0, 6.3, nf), np.full(N, 2 / bin), sampleRate=1e9)


def one_fewer(N, bin, start):
    """one bin fewer than fits, so that samples are left over behind the last bin (the whole record: its one bin)"""
    return max((N - start) // bin - 1, 1)


def assert_parity(got, x, e, bin, start, bins, what=''):
    want = ref.binned(x, e, bin, start, bins)
    bound = 1e-12 * ref.magnitude(x, e, bin, start, bins)
    err = np.abs(got - want)
    assert got.shape == want.shape and got.dtype == np.complex128, (got.shape, want.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        print(what, 'max err / bound:', float(np.max(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
    assert np.all(err <= bound), (what, float(np.max(err - bound)), np.unravel_index(np.argmax(err - bound), err.shape))


def run(bd, x):
    return bd.apply_torch(torch.from_numpy(x).to(DEV)).cpu().numpy()


F64, F32, I16 = np.float64, np.float32, np.int16
# (dtype, nf, S, N, bin, start): every dtype, nf in {1, 5, 8, 9, 33} (the bucket edges, more than one column block),
# S in {1, 63, 64, 65, 130}, N in {1000, 4096}, (bin, start) in {(1, 0), (3, 1), (16, 0), (17, 5), (100, 3), (128, 0),
# (N, 0)}: each value of each axis with each dtype at least once, not the cross product
PARITY = [
    (F64, 1, 1, 1000, 1, 0), (F32, 5, 63, 1000, 3, 1), (I16, 8, 64, 4096, 16, 0), (F64, 9, 65, 1000, 17, 5),
    (F32, 33, 130, 1000, 100, 3), (I16, 5, 130, 4096, 128, 0), (F64, 8, 64, 4096, 4096, 0), (I16, 33, 1, 4096, 17, 5),
    (F32, 1, 65, 4096, 1, 0), (I16, 9, 63, 1000, 100, 3), (F64, 5, 130, 4096, 3, 1), (F32, 8, 1, 1000, 1000, 0),
    (I16, 1, 64, 1000, 3, 1), (F64, 33, 63, 4096, 128, 0), (F32, 9, 130, 4096, 16, 0), (I16, 8, 65, 1000, 128, 0),
    (F64, 8, 130, 4096, 100, 3), (F32, 5, 64, 4096, 17, 5), (I16, 5, 1, 1000, 1, 0), (F64, 1, 63, 1000, 16, 0),
    (F32, 33, 65, 1000, 128, 0), (I16, 9, 130, 1000, 1000, 0), (F64, 9, 1, 4096, 100, 3), (I16, 33, 64, 1000, 16, 0),
]


@pytest.mark.parametrize('dtype,nf,S,N,bin,start', PARITY, ids=lambda v: getattr(v, '__name__', str(v)))
def test_parity(dtype, nf, S, N, bin, start):
    rng = np.random.default_rng(nf * 1000003 + N * 31 + S * 7 + bin * 13 + np.dtype(dtype).itemsize)
    bins = one_fewer(N, bin, start)
    e = tones(rng, nf, N, bin)
    x = traces(rng, S, N, dtype)
    bd = BinnedDemodulator.from_matrix(e, bin, start, bins, dtype)
    got = run(bd, x)
    assert got.shape == (S, bins, nf)
    assert_parity(got, x, e, bin, start, bins, f'{np.dtype(dtype)} nf={nf} S={S} N={N} bin={bin} start={start}')
    assert bd.kernel_name(S) == 'bdemod_tile<%s,%d> groups=%d' % (
        TYPE_NAME[np.dtype(dtype)], 4 if nf <= 4 else 8 if nf <= 8 else 16 if nf <= 16 else 32, ref.bin_groups(S, nf, bins))
    bd.close()


def test_all_bins_that_fit_and_the_numpy_door():
    """bins=None, a record the bins fill to the last sample, and __call__ on (N,) and (2, 3, N) signals"""
    rng = np.random.default_rng(21)
    N, bin = 1024, 128
    f = [37e6, -101e6, 250e6]
    bd = BinnedDemodulator(f, N, bin, phaseList=[0.1, 0.2, 0.3])
    e = getFTMatrix(f, N, [0.1, 0.2, 0.3], np.full(N, 2 / bin))
    assert bd.bins == 8
    sig = rng.normal(size=N)
    r1 = bd(sig)
    assert r1.shape == (8, 3)
    assert_parity(r1[None], sig[None], e, bin, 0, 8, 'call 1-D')
    sig3 = rng.normal(size=(2, 3, N))
    r3 = bd(sig3)
    assert r3.shape == (2, 3, 8, 3)
    assert_parity(r3.reshape(6, 8, 3), sig3.reshape(6, N), e, bin, 0, 8, 'call 3-D')
    # a steady tone reads A exp(i phi) in every bin: 37 MHz is no whole number of periods per bin, so to the leakage
    t = np.arange(N) / 1e9
    tone = 0.7 * np.cos(2 * np.pi * 250e6 * t + 0.9)                  # 32 periods per bin
    assert np.allclose(BinnedDemodulator([250e6], N, bin)(tone)[:, 0], 0.7 * np.exp(0.9j), rtol=0, atol=1e-12)
    assert bd.apply_torch(torch.zeros((0, N), dtype=torch.float64, device=DEV)).shape == (0, 8, 3)
    bd.close()


def test_integer_sums_are_exact():
    """int16 codes times a matrix of small integers: every sum is an integer far below 2^53, so the device and the
    referee agree bit for bit -- an off-by-one at a bin edge cannot hide"""
    rng = np.random.default_rng(22)
    S, N, nf, bin, start = 130, 1000, 5, 100, 3
    e = (rng.integers(-3, 4, (N, nf)) + 1j * rng.integers(-3, 4, (N, nf))).astype(np.complex128)
    x = traces(rng, S, N, np.int16)
    for bins in (9, 8, 1):
        got = run(BinnedDemodulator.from_matrix(e, bin, start, bins, np.int16), x)
        want = ref.binned(x, e, bin, start, bins)
        assert np.all(want.real == np.round(want.real)) and np.abs(want.real).max() < 2.0 ** 53
        assert bits_equal(got + 0.0, want + 0.0), bins                 # (+ 0.0: the sign of a zero sum is nobody's)
        assert np.array_equal(got, want)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_nan_stays_in_its_bin(dtype):
    rng = np.random.default_rng(23)
    S, N, nf, bin, start, bins = 70, 1000, 9, 100, 3, 8
    e = tones(rng, nf, N, bin)
    x = traces(rng, S, N, dtype)
    bd = BinnedDemodulator.from_matrix(e, bin, start, bins, dtype)
    clean = run(bd, x)
    # a NaN before `start`, one behind the last bin, an Inf in the very last sample: nothing changes
    y = x.copy()
    y[5, 0], y[5, 2], y[66, start + bins * bin], y[9, N - 1] = np.nan, np.inf, np.nan, -np.inf
    assert bits_equal(run(bd, y), clean)
    # a NaN inside a bin -- its first sample, its last, one in the middle -- changes that (shot, bin) and no other bit
    for s, k in ((0, start), (69, start + bins * bin - 1), (33, start + 3 * bin + 41), (64, start + 4 * bin),
                 (63, start + 4 * bin - 1)):
        y = x.copy()
        y[s, k] = np.nan
        got = run(bd, y)
        w = ref.bin_of(k, bin, start, bins)
        assert np.all(np.isnan(got[s, w].real) & np.isnan(got[s, w].imag)), (s, k)
        got[s, w] = clean[s, w]
        assert bits_equal(got, clean), (s, k)
    y = x.copy()
    y[7, start + 2 * bin + 1] = np.inf                              # an Inf: the same, and the referee says what it gives
    got = run(bd, y)
    assert not np.isfinite(got[7, 2]).any()
    got[7, 2] = clean[7, 2]
    assert bits_equal(got, clean)
    bd.close()


def shot_view(win, bins, nf):
    """a (shots, bins * nf) window as the (shots, bins, nf) tensor apply_torch takes: dense within a shot"""
    return win.as_strided((win.shape[0], bins, nf), (win.stride(0), nf, 1))


@pytest.mark.parametrize('dtype', [np.int16, np.float32, np.float64])
@pytest.mark.parametrize('S,N,bin,start', [(50, 1000, 100, 3), (130, 1031, 16, 0), (65, 1000, 17, 5)])
def test_row_windows(dtype, S, N, bin, start):
    """traces as a window at an odd element and an odd row stride (no 16-byte alignment to lean on, another alignment
    in every row), out as a window with a shot stride above bins * nf: parity, the bits of an apply on dense tensors,
    every guard intact"""
    rng = np.random.default_rng(24 + S)
    nf, bins = 5, one_fewer(N, bin, start)
    e = tones(rng, nf, N, bin)
    x = traces(rng, S, N, dtype)
    x[:, :start] = 0 if dtype == np.int16 else np.nan                # what lies outside the bins is not read ...
    bd = BinnedDemodulator.from_matrix(e, bin, start, bins, dtype)
    src = Window(S, N, dtype, x)                                       # ... nor is the sentinel around the window
    dst = Window(S, bins * nf, np.complex128)
    out = shot_view(dst.win, bins, nf)
    assert out.stride(0) > bins * nf
    res = bd.apply_torch(src.win, out)
    assert res.data_ptr() == dst.ptr
    got = dst.host().reshape(S, bins, nf)
    assert_parity(got, x, e, bin, start, bins, f'window {np.dtype(dtype)} S={S} bin={bin}')
    dst.assert_guards()
    src.assert_holds(x)
    assert bits_equal(run(bd, x), got)                                 # the order of additions does not depend on where the rows lie
    bd.close()


def test_far_rows():
    """two shots more than 2^32 elements apart: s * ldx in 64 bits"""
    rng = np.random.default_rng(25)
    N, nf, bin, start = 2 * 2048 + 5, 5, 100, 3
    bins = one_fewer(N, bin, start)
    e = tones(rng, nf, N, bin)
    x = traces(rng, 2, N, np.int16)
    src = FarWindow(N, np.int16, x)
    bd = BinnedDemodulator.from_matrix(e, bin, start, bins, np.int16)
    got = bd.apply_torch(src.win)
    torch.cuda.synchronize()
    assert_parity(got.cpu().numpy(), x, e, bin, start, bins, 'far rows')
    src.assert_holds(x)
    bd.close()


def test_refused_tensors_on_the_device():
    S, N, nf, bin, bins = 6, 64, 2, 16, 4
    bd = BinnedDemodulator([10e6, 20e6], N, bin)
    arena = torch.zeros(4096, dtype=torch.float64, device=DEV)
    x = arena[:S * N].view(S, N)
    out = torch.view_as_complex(arena[1024:1024 + 2 * S * bins * nf].view(S, bins, nf, 2))
    assert bd.apply_torch(x, out).data_ptr() == out.data_ptr()
    good = torch.zeros((S, N), dtype=torch.float64, device=DEV)
    for bad in (good[:, :N - 1], good.to(torch.float32), good.cpu(), torch.zeros((N, S), dtype=torch.float64, device=DEV).t(),
                good[0]):
        with pytest.raises(ValueError, match='traces must be'):
            bd.apply_torch(bad)
    with pytest.raises(ValueError, match='complex traces'):
        bd.apply_torch(good.to(torch.complex128))
    for bad_out in (torch.zeros((S, bins, nf + 1), dtype=torch.complex128, device=DEV),
                    torch.zeros((S, bins, nf), dtype=torch.complex64, device=DEV),
                    torch.zeros((S - 1, bins, nf), dtype=torch.complex128, device=DEV),
                    torch.zeros((S, bins * nf), dtype=torch.complex128, device=DEV),
                    torch.zeros((S, bins, nf), dtype=torch.complex128),
                    torch.zeros((S, bins, nf + 1), dtype=torch.complex128, device=DEV)[:, :, :nf],
                    torch.zeros((S, nf, bins), dtype=torch.complex128, device=DEV).transpose(1, 2)):
        with pytest.raises(ValueError, match='out must be'):
            bd.apply_torch(good, bad_out)
    # the library's own refusals, through the raw pointers: nothing is launched
    X, O, W = x.data_ptr(), out.data_ptr(), bins * nf
    for args, message in (((None, S, N, O, W), 'null traces / out'), ((X, S, N, None, W), 'null traces / out'),
                          ((X, -1, N, O, W), 'n_shots < 0'), ((X, S, N - 1, O, W), 'traces row stride smaller'),
                          ((X, S, N, O, W - 1), 'out row stride smaller'), ((X + 4, S, N, O, W), 'not aligned to their element'),
                          ((X, S, N, O + 8, W), 'not aligned to their element'),
                          ((X, S, N, X + 16 * 8, W), 'out overlaps traces'),
                          ((X, S, N, X + 8 * (S * N - 2), W), 'out overlaps traces')):
        with pytest.raises(RuntimeError, match=message):
            bd.plan.apply(*args)
    bd.plan.apply(None, 0, N, None, W)                                # no shots: nothing is looked at, nothing enqueued
    bd.plan.apply(X, 1, 1, O, W)                                      # a lone trace's stride is read by no kernel
    torch.cuda.synchronize()
    bd.close()


def test_two_applies_and_a_side_stream_are_bitwise_equal():
    rng = np.random.default_rng(26)
    for dtype, S, N, nf, bin, start in ((np.float32, 1000, 4096, 8, 128, 0), (np.float64, 3, 4096, 33, 100, 3)):
        e = tones(rng, nf, N, bin)
        x_host = traces(rng, S, N, dtype)
        x = torch.from_numpy(x_host).to(DEV)
        bd = BinnedDemodulator.from_matrix(e, bin, start, None, dtype)
        a = bd.apply_torch(x).cpu().numpy()
        b = bd.apply_torch(x).cpu().numpy()
        assert bits_equal(a, b)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = bd.apply_torch(torch.from_numpy(x_host).to(DEV)).clone()
        side.synchronize()
        assert bits_equal(a, c.cpu().numpy())
        assert_parity(a, x_host, e, bin, start, bd.bins, f'streams {np.dtype(dtype)}')
        bd.close()


@pytest.mark.parametrize('dtype,S,bin,start', [(np.int16, 130, 100, 3), (np.float64, 40, 16, 0)],
                         ids=lambda v: getattr(v, '__name__', str(v)))
def test_graph_replay(dtype, S, bin, start):
    """one apply captured and replayed on A, B, A: each replay gives the bits of an eager twin plan, is within the
    bound of the referee, and leaves no sentinel"""
    N, nf = 1000, 5
    bins = one_fewer(N, bin, start)
    rng = np.random.default_rng(27)
    e = tones(rng, nf, N, bin)
    feeds = [(traces(rng, S, N, dtype), ) for _ in range(2)]

    def make():
        bd = BinnedDemodulator.from_matrix(e, bin, start, bins, dtype)
        x = torch.empty((S, N), dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device=DEV)
        out = torch.empty((S, bins, nf), dtype=torch.complex128, device=DEV)
        bd.apply_torch(x, out)                                         # (the plan is made outside the capture)
        return bd, (lambda: bd.apply_torch(x, out)), [x], [out]

    bd, run_, statics, outputs = make()
    twin, trun, tstatics, toutputs = make()
    got = replay(run_, statics, [feeds[0], feeds[1], feeds[0]], outputs)
    for k, (out, ) in enumerate(got):
        feed = feeds[k % 2]
        t_out, = eager(trun, tstatics, feed, toutputs)
        assert bits_equal(out, t_out), k
        assert sentinels_left(out) == 0, k
        assert_parity(out, feed[0], e, bin, start, bins, f'replay {k}')
    bd.close()
    twin.close()


def test_sum_over_bins_meets_the_demodulator():
    """start = 0 and bins * bin = N: the bins of a shot, summed and rescaled by bin / N, are the demodulator's point
    within the sum of both bounds (the weights are 2 / bin here and 2 / N there, exactly bin / N apart for bin = 128)"""
    rng = np.random.default_rng(28)
    S, N, bin = 200, 4096, 128
    f = rng.uniform(-400e6, 400e6, 8)
    x = traces(rng, S, N, np.int16)
    xt = torch.from_numpy(x).to(DEV)
    bd = BinnedDemodulator(f, N, bin, dtype=np.int16)
    dm = Demodulator(f, N, dtype=np.int16)
    assert bd.bins * bin == N
    traj = bd.apply_torch(xt).cpu().numpy()
    iq = dm.apply_torch(xt).cpu().numpy()
    x64 = x.astype(np.float64)
    bound = 1e-12 * (ref.magnitude(x, bd.e, bin).sum(axis=1) * bin / N + np.abs(x64) @ np.abs(dm.e))
    err = np.abs(traj.sum(axis=1) * bin / N - iq)
    print('sum over bins against the demodulator, max err / bound:', float(np.max(err / bound)))
    assert np.all(err <= bound)
    bd.close()
    dm.close()


def test_a_bin_feeds_the_state_discriminator():
    """out[:, w] is an (S, nf) points matrix as StateDiscriminator.apply_torch takes it: the labels of classify_points
    on the host copy of that bin"""
    rng = np.random.default_rng(29)
    S, N, bin, nf = 300, 1000, 100, 3
    f = np.array([50e6, 120e6, -200e6])
    t = np.arange(N) / 1e9
    state = rng.integers(0, 2, (S, nf))
    amp = np.where(state == 0, 0.3, 0.8)
    x = (amp[:, :, None] * np.cos(2 * np.pi * f[None, :, None] * t)).sum(axis=1) + 0.05 * rng.normal(size=(S, N))
    bd = BinnedDemodulator(f, N, bin, start=3)
    traj = bd.apply_torch(torch.from_numpy(x).to(DEV))
    centres = np.stack([np.full(nf, 0.3 + 0j), np.full(nf, 0.8 + 0j)], axis=1)
    sd = StateDiscriminator(centres)
    host = traj.cpu().numpy()
    for w in (0, 4, bd.bins - 1):
        pts = traj[:, w]
        assert tuple(pts.shape) == (S, nf) and pts.stride(0) == bd.bins * nf
        labels = sd.apply_torch(pts).cpu().numpy()
        assert np.array_equal(labels, classify_points(host[:, w], centres)), w
        assert np.array_equal(labels, state), w                        # (and they are the states that were played)
    sd.close()
    bd.close()


def test_kernel_name_shows_the_bin_groups():
    bd = BinnedDemodulator.from_matrix(getFTMatrix([1e6] * 9, 4096), 16, dtype=np.int16)
    assert bd.bins == 256
    for S in (1, 64, 65, 130, 4096, 65536):
        groups = _engine.bdemod_bin_groups(S, 9, 256)
        assert groups == ref.bin_groups(S, 9, 256)
        assert bd.kernel_name(S) == 'bdemod_tile<short,16> groups=%d' % groups
    assert bd.kernel_name(1) == 'bdemod_tile<short,16> groups=64' and bd.kernel_name(65536).endswith('groups=1')
    bd.close()


def test_plain_c_consumer_demodulates_bins(tmp_path):
    exe = tmp_path / 'bdemod_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'bdemod_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'bdemod_smoke: bdemod_tile<short,4> groups=4, 19 bins per shot on the device, parity ok' in r.stdout, r.stdout
