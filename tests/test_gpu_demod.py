"""Readout demodulation on the device (waveforms_amd.utils.Demodulator, csrc/wfk_demod.hip) against host NumPy:
|device - x.astype(float64) @ e| <= 1e-12 * (|x| @ |e|) element by element, over trace dtypes, tone counts
(column buckets and blocks), record lengths (tails, split-K) and shot counts; windows, strided outputs,
streams, determinism, NaN isolation, a sampler -> demodulator loopback and the plain-C consumer."""
import os
import subprocess

import numpy as np
import pytest
import torch

import waveforms_amd as wf
from waveforms_amd.utils import Demodulator, getFTMatrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda', 0)


def traces(rng, S, N, dtype):
    if np.dtype(dtype) == np.int16:
        return rng.integers(-32768, 32768, size=(S, N), dtype=np.int16)
    return rng.normal(size=(S, N)).astype(dtype)


def tones(rng, nf, N):
    return getFTMatrix(rng.uniform(-400e6, 400e6, nf), N, rng.uniform(0, 6.3, nf), sampleRate=1e9)


def assert_parity(got, x, e):
    x64 = np.asarray(x, dtype=np.float64)
    want = x64 @ e
    bound = 1e-12 * (np.abs(x64) @ np.abs(e))
    err = np.abs(got - want)
    assert got.shape == want.shape and got.dtype == np.complex128
    assert np.all(err <= bound), (np.max(err - bound), np.unravel_index(np.argmax(err - bound), err.shape))


def run(dm, x):
    return dm.apply_torch(torch.from_numpy(x).to(DEV)).cpu().numpy()


# (dtype, nf, N, S): a covering subset of dtypes x nf {1,2,8,16,32,33,100} x N {1,7,1000,4096,4097,100000}
# x S {1,3,64,1000}
PARITY = [
    (np.float64, 1, 1, 1), (np.float32, 2, 7, 3), (np.int16, 8, 1000, 64), (np.float64, 16, 4096, 1000),
    (np.float32, 32, 4097, 64), (np.int16, 33, 1000, 3), (np.float64, 100, 4097, 3), (np.int16, 1, 100000, 1),
    (np.float32, 8, 100000, 3), (np.float64, 2, 7, 1000), (np.int16, 16, 4096, 1), (np.float64, 32, 1, 64),
    (np.float32, 1, 4096, 1000), (np.int16, 100, 7, 1000), (np.float64, 8, 100000, 64), (np.float32, 33, 1000, 1),
    (np.int16, 2, 4097, 64), (np.float64, 1, 1000, 3), (np.float32, 16, 1, 3), (np.int16, 32, 100000, 3),
]


@pytest.mark.parametrize('dtype,nf,N,S', PARITY, ids=lambda v: getattr(v, '__name__', str(v)))
def test_parity(dtype, nf, N, S):
    rng = np.random.default_rng(nf * 1000003 + N * 31 + S * 7 + np.dtype(dtype).itemsize)
    e = tones(rng, nf, N)
    x = traces(rng, S, N, dtype)
    dm = Demodulator.from_matrix(e, dtype)
    assert_parity(run(dm, x), x, e)


@pytest.mark.parametrize('dtype', [np.float64, np.int16])
def test_d1_full_size(dtype):
    S, N, nf = 65536, 4096, 8
    rng = np.random.default_rng(1)
    e = tones(rng, nf, N)
    xt = torch.randn(S, N, dtype=torch.float64, device=DEV) if dtype == np.float64 else \
        torch.randint(-32768, 32768, (S, N), dtype=torch.int16, device=DEV)
    dm = Demodulator.from_matrix(e, dtype)
    assert '+' not in dm.kernel_name(S)          # one launch fills the chip
    got = dm.apply_torch(xt)
    rows = np.r_[0, 1, S - 1, rng.choice(S, 64, replace=False)]
    idx = torch.from_numpy(rows).to(DEV)
    assert_parity(got[idx].cpu().numpy(), xt[idx].cpu().numpy(), e)


def test_window_and_strided_out():
    rng = np.random.default_rng(2)
    S, N, nf = 300, 1000, 5
    e = tones(rng, nf, N)
    for dtype in (np.float64, np.float32, np.int16):
        wide = traces(rng, S, N + 257, dtype)
        dm = Demodulator.from_matrix(e, dtype)
        xt = torch.from_numpy(wide).to(DEV)
        for w0 in (100, 101):                        # 16-B aligned and unaligned row starts
            out_wide = torch.full((S, nf + 3), complex(7, 7), dtype=torch.complex128, device=DEV)
            out = out_wide[:, 1:1 + nf]
            r = dm.apply_torch(xt[:, w0:w0 + N], out)
            assert r.data_ptr() == out.data_ptr()
            ow = out_wide.cpu().numpy()
            assert_parity(ow[:, 1:1 + nf], wide[:, w0:w0 + N], e)
            assert np.all(ow[:, 0] == 7 + 7j) and np.all(ow[:, 1 + nf:] == 7 + 7j)


def test_two_applies_are_bitwise_equal():
    rng = np.random.default_rng(3)
    for S, N in ((1000, 4096), (3, 100000)):          # one launch, split-K
        e = tones(rng, 8, N)
        x = torch.from_numpy(traces(rng, S, N, np.float32)).to(DEV)
        dm = Demodulator.from_matrix(e, np.float32)
        a = dm.apply_torch(x).cpu().numpy()
        b = dm.apply_torch(x).cpu().numpy()
        assert np.array_equal(a.view(np.float64), b.view(np.float64))


def test_non_default_stream():
    rng = np.random.default_rng(4)
    S, N = 2000, 4096
    e = tones(rng, 4, N)
    x_host = traces(rng, S, N, np.int16)
    dm = Demodulator.from_matrix(e, np.int16)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        x = torch.from_numpy(x_host).to(DEV, non_blocking=False)
        out = dm.apply_torch(x)
        y = out.clone()
    s.synchronize()
    assert_parity(y.cpu().numpy(), x_host, e)


def test_split_k_one_long_record():
    N = 10**7
    rng = np.random.default_rng(5)
    e = getFTMatrix([12.5e6], N, [0.3])
    x = rng.normal(size=(1, N))
    dm = Demodulator.from_matrix(e)
    assert dm.kernel_name(1).endswith('demod_reduce')
    xt = torch.from_numpy(x).to(DEV)
    a = dm.apply_torch(xt).cpu().numpy()
    assert_parity(a, x, e)
    assert np.array_equal(a, dm.apply_torch(xt).cpu().numpy())


def test_nan_stays_in_its_row():
    rng = np.random.default_rng(6)
    for S, N in ((200, 4096), (5, 50000)):
        e = tones(rng, 3, N)
        x = traces(rng, S, N, np.float64)
        x[2, N // 3] = np.nan
        got = run(Demodulator.from_matrix(e), x)
        assert np.all(np.isnan(got[2]))
        keep = np.arange(S) != 2
        assert np.all(np.isfinite(got[keep]))
        assert_parity(got[keep], x[keep], e)


def test_call_numpy_shapes():
    rng = np.random.default_rng(7)
    N = 777
    dm = Demodulator([10e6, 20e6, 30e6], N, [0.1, 0.2, 0.3])
    e = getFTMatrix([10e6, 20e6, 30e6], N, [0.1, 0.2, 0.3])
    sig = rng.normal(size=N)
    r1 = dm(sig)
    assert r1.shape == (3,)
    assert_parity(r1[None], sig[None], e)
    sig3 = rng.normal(size=(2, 4, N))
    r3 = dm(sig3)
    assert r3.shape == (2, 4, 3)
    assert_parity(r3.reshape(8, 3), sig3.reshape(8, N), e)
    with pytest.raises(ValueError):
        dm(sig[:-1])
    with pytest.raises(ValueError):
        dm(sig + 1j)
    with pytest.raises(ValueError):
        Demodulator([1e6], N, dtype=np.int16)(sig)         # float64 samples do not fit an int16 demodulator


def test_apply_torch_validation():
    dm = Demodulator([1e6, 2e6], 100, dtype=np.float32)
    good = torch.zeros(4, 100, dtype=torch.float32, device=DEV)
    for bad in (torch.zeros(4, 99, dtype=torch.float32, device=DEV), torch.zeros(4, 100, device=DEV,
                dtype=torch.float64), torch.zeros(4, 100, dtype=torch.float32),
                torch.zeros(200, 4, dtype=torch.float32, device=DEV).t(),
                torch.zeros(4, 100, dtype=torch.complex64, device=DEV), torch.zeros(100, dtype=torch.float32,
                                                                                   device=DEV)):
        with pytest.raises(ValueError):
            dm.apply_torch(bad)
    for bad_out in (torch.zeros(4, 3, dtype=torch.complex128, device=DEV),
                    torch.zeros(4, 2, dtype=torch.complex64, device=DEV),
                    torch.zeros(3, 2, dtype=torch.complex128, device=DEV)):
        with pytest.raises(ValueError):
            dm.apply_torch(good, bad_out)
    assert dm.apply_torch(good[:0]).shape == (0, 2)


def test_loopback_sampler_to_demodulator():
    """BatchSampler puts tones on FFT bins onto a device tensor; the demodulator reads A_k e^{i phi_k} back."""
    from waveforms_amd._sampling import BatchSampler
    sr, N = 1e9, 4096
    m = np.array([37, 101, 500, 1234, 1900])
    f = m * sr / N
    rng = np.random.default_rng(8)
    S = 6
    A = rng.uniform(0.05, 0.3, (S, len(m)))
    phi = rng.uniform(-3, 3, (S, len(m)))
    chans = []
    for s in range(S):
        w = wf.zero()
        for k in range(len(m)):
            w = w + A[s, k] * wf.cos(2 * np.pi * f[k], phi[s, k])
        chans.append(w)
    bs = BatchSampler(chans, ('linspace', 0.0, N / sr, N, False))
    y = torch.empty(S, N, dtype=torch.float64, device=DEV)
    bs.launch_torch(y)
    dm = Demodulator(f, N, sampleRate=sr)
    got = dm.apply_torch(y).cpu().numpy()
    want = A * np.exp(1j * phi)
    tol = 1e-9 * A.sum(axis=1, keepdims=True)
    assert np.all(np.abs(got - want) <= tol), np.max(np.abs(got - want))
    assert_parity(got, y.cpu().numpy(), getFTMatrix(f, N, sampleRate=sr))


def test_shift_fractional_delay_matches_host_formula():
    from waveforms_amd.utils import shift
    sig = np.random.default_rng(9).normal(size=300)
    for d in (0.3e-9, 2.7e-9, -1.25e-9):
        points = int(d // 1e-9)
        delta = d / 1e-9 - points
        want = np.convolve(sig, np.array([0, 1 - delta, delta]), mode='same')
        ret = np.zeros_like(want)
        if points < 0:
            ret[:points] = want[-points:]
        elif points > 0:
            ret[points:] = want[:-points]
        else:
            ret = want
        assert np.max(np.abs(shift(sig, d, 1e-9) - ret)) <= 1e-12


def test_plain_c_consumer_demodulates_int16(tmp_path):
    exe = tmp_path / 'demod_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'demod_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'demodulated on the device, parity ok' in r.stdout, r.stdout
