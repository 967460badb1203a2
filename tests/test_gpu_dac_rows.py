"""The DAC stage on the device (distortion.DacStage / dac_codes_rows, csrc/wfk_dac_rows.hip) against the referee
tests/dac_rows_ref.py, the NumPy statement of the semantics.  Codes and counts are integers and the formula rounds a
product and then a sum without fusing them, as NumPy does: every comparison here is exact, there is no tolerance."""
import os
import subprocess

import numpy as np
import pytest
import torch

import dac_rows_ref as ref
from waveforms_amd import distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 8191, 8192, 8193, 10007]   # 8192 codes: one workgroup's span
FORMATS = [(16, 0), (14, 2), (12, 0), (2, 14)]                                   # (bits, shift)
NP_OF = {'f64': np.float64, 'f32': np.float32}
NAME_OF = {'f64': 'double', 'f32': 'float'}
SENTINEL = -21846                                                                # 0xAAAA


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def rows_input(rows, n, seed, dtype=np.float64, over=1.2, specials=True):
    """samples in [-over, over] of full scale 1 (over > 1: some past each rail), with +-inf, NaN and -0.0 in them"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-over, over, (rows, n))
    if specials:
        flat = x.reshape(-1)
        for start, step, v in ((0, 7, np.inf), (1, 11, -np.inf), (2, 13, np.nan), (3, 17, -0.0)):
            flat[start % flat.size::step * max(1, flat.size // 97)] = v
    return x.astype(dtype)


def gains_offsets(rows, bits):
    """gains of both signs around hi per unit, offsets of both signs, fractional ones among them"""
    hi = 2**(bits - 1) - 1
    g = np.array([1.0, -1.0, 0.5, -0.37, 1.0, 0.93])[np.arange(rows) % 6] * hi
    o = np.array([0.0, 12.5, -300.25, 0.5, hi / 2, -hi / 3])[np.arange(rows) % 6]
    return g, o


def run(x, g, o, bits=16, shift=0, k=1, counts=True):
    """x (rows, n) NumPy -> (codes, counts or None) of a stage built for it, counts from a tensor full of garbage"""
    st = distortion.DacStage(g, x.shape[1], offset=o, bits=bits, shift=shift, interleave=k, dtype=x.dtype)
    try:
        c = torch.full((x.shape[0], 3), 0x5a5a5a5a5a, dtype=torch.int64, device=dev()) if counts else None
        y = st.apply_torch(torch.from_numpy(x).to(dev()), counts=c)
        assert y.dtype == torch.int16 and tuple(y.shape) == (st.out_rows, st.out_n)
        return y.cpu().numpy(), (c.cpu().numpy() if counts else None)
    finally:
        st.close()


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}')


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', SIZES)
def test_small_shapes(n, kind):
    rows = 6
    x = rows_input(rows, n, 100 + n, NP_OF[kind])
    for bits, shift in FORMATS:
        g, o = gains_offsets(rows, bits)
        for k in (1, 2):
            st = distortion.DacStage(g, n, offset=o, bits=bits, shift=shift, interleave=k, dtype=NP_OF[kind])
            assert st.kernel_name() == f'dac_rows<{NAME_OF[kind]}>'
            assert st.kernel_name(counts=True) == f'dac_rows_count<{NAME_OF[kind]}>'
            assert (st.lo, st.hi, st.n, st.batch) == (-2**(bits - 1), 2**(bits - 1) - 1, n, rows)
            assert (st.out_rows, st.out_n) == (rows // k, k * n)
            st.close()
            codes, counts = run(x, g, o, bits, shift, k)
            want, want_counts = ref.dac_ref(x, g, o, bits, shift, k)
            same(codes, want, f'codes n={n} {kind} bits={bits} shift={shift} k={k}')
            same(counts, want_counts, f'counts n={n} {kind} bits={bits} shift={shift} k={k}')
            if n >= 255 and bits == 16:                      # the case does clip, on both rails, and has NaNs
                assert want_counts[:, 0].sum() > 0 and want_counts[:, 1].sum() > 0 and want_counts[:, 2].sum() > 0


def test_rounding_sensitive_rows():
    """exact ties after two roundings: a contracted multiply-add or round-half-away gives other codes on hundreds of
    these samples (tests/test_dac_rows_cpu.py holds the builder to that)"""
    gq, M = 9731.37, 20000
    x, ks = ref.sensitive_row(1024, gq, M, seed=7)
    for k in (1, 2):
        xx = np.stack([x, x[::-1].copy()])
        codes, counts = run(xx, [gq, gq], [-float(M), -float(M)], k=k)
        want, want_counts = ref.dac_ref(xx, [gq, gq], [-float(M), -float(M)], interleave=k)
        same(codes, want, f'sensitive rows k={k}')
        assert not counts.any() and not want_counts.any()
    assert np.array_equal(ref.dac_ref(x[None], gq, -float(M))[0][0], np.rint(ks + 0.5).astype(np.int16))
    x32, ks32, g32 = ref.tie_row32()
    for off in (0.0, 7.0, -20000.0):
        codes, counts = run(x32[None], [g32], [off])
        assert np.array_equal(codes[0], np.rint(ks32 + 0.5 + off).astype(np.int16)) and not counts.any()
        same(codes, ref.dac_ref(x32[None], g32, off)[0], f'float32 ties offset={off}')


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('n', [5, 256, 4099])
def test_windows_and_canaries(n, k, kind):
    """every output lead 0 .. 7 codes (odd ones under k = 2 too), input rows 8 and 40 bytes into a wider buffer with
    stride n + 37, output stride k n + 64: sentinels before, after and between the output rows stay, the input is
    intact bit for bit, a counts tensor full of garbage comes out exact and a second apply does not add to it"""
    dtype = NP_OF[kind]
    tdt = torch.float64 if kind == 'f64' else torch.float32
    rows = 6
    x = rows_input(rows, n, 400 + n, dtype)
    g, o = gains_offsets(rows, 14)
    st = distortion.DacStage(g, n, offset=o, bits=14, shift=2, interleave=k, dtype=dtype)
    want, want_counts = ref.dac_ref(x, g, o, 14, 2, k)
    raw = np.uint64 if kind == 'f64' else np.uint32
    for off_bytes in (8, 40):
        off = off_bytes // np.dtype(dtype).itemsize
        wide = torch.full((rows, n + 37), 7.0, dtype=tdt, device=dev())
        win = wide[:, off:off + n]
        win.copy_(torch.from_numpy(x))
        before = wide.cpu().numpy().view(raw).copy()
        for lead in range(8):
            out = torch.full((rows // k, k * n + 64), SENTINEL, dtype=torch.int16, device=dev())
            counts = torch.full((rows, 3), -77, dtype=torch.int64, device=dev())
            res = st.apply_torch(win, out[:, lead:lead + k * n], counts)
            assert res.data_ptr() == out[:, lead:].data_ptr() and tuple(res.shape) == (rows // k, k * n)
            full = out.cpu().numpy()
            same(full[:, lead:lead + k * n], want, f'window n={n} k={k} {kind} lead={lead} off={off_bytes}')
            assert np.all(full[:, :lead] == SENTINEL) and np.all(full[:, lead + k * n:] == SENTINEL)
            same(counts.cpu().numpy(), want_counts, f'counts n={n} k={k} {kind} lead={lead}')
            st.apply_torch(win, out[:, lead:lead + k * n], counts)                  # overwrites, does not accumulate
            same(counts.cpu().numpy(), want_counts, f'counts of a second apply n={n} k={k} {kind} lead={lead}')
        assert np.array_equal(wide.cpu().numpy().view(raw), before)
    st.close()


@pytest.mark.parametrize('kind,k', [('f64', 1), ('f64', 2), ('f32', 2)])
def test_many_workgroups_per_row(kind, k):
    """64 x 100003: a few percent of the samples past each rail, scattered NaNs; counts exact per input row, and under
    k = 2 the two input rows of an output row have counts of their own"""
    rows, n = 64, 100003
    rng = np.random.default_rng(700)
    x = rows_input(rows, n, 701, NP_OF[kind], over=1.03, specials=False)
    x[rng.integers(0, rows, 500), rng.integers(0, n, 500)] = np.nan
    x[1::2, ::3] *= 0.9                                                              # the Q rows clip less
    g = np.array([32767.0, -32767.0, 32767.0, 32767.0])[np.arange(rows) % 4]
    o = np.array([0.0, 12.5, -300.25, 0.5])[np.arange(rows) % 4]
    codes, counts = run(x, g, o, k=k)
    want, want_counts = ref.dac_ref(x, g, o, interleave=k)
    same(codes, want, f'{rows} x {n} {kind} k={k}')
    same(counts, want_counts, f'counts {rows} x {n} {kind} k={k}')
    assert want_counts[:, :2].min() > 100 and want_counts[:, 2].sum() >= 490
    assert all(tuple(want_counts[r]) != tuple(want_counts[r + 1]) for r in range(0, rows, 2))


@pytest.mark.parametrize('n', [257, 10007])
def test_row_independence(n):
    """a row's codes and counts are the same alone, first and last in a batch, and as the I or the Q of a pair"""
    x = rows_input(1, n, 500 + n)
    others = rows_input(4, n, 501 + n)
    g0, o0 = 29000.5, -17.25
    og, oo = [31000.0, -8000.0, 123.0, -32767.0], [0.0, 5.5, -3.0, 100.0]
    alone, c_alone = run(x, [g0], [o0])
    want, want_counts = ref.dac_ref(x, g0, o0)
    same(alone, want, 'alone')
    same(c_alone, want_counts, 'alone, counts')
    first, c_first = run(np.vstack([x, others]), [g0] + og, [o0] + oo)
    last, c_last = run(np.vstack([others, x]), og + [g0], oo + [o0])
    assert np.array_equal(first[0], alone[0]) and np.array_equal(c_first[0], c_alone[0])
    assert np.array_equal(last[4], alone[0]) and np.array_equal(c_last[4], c_alone[0])
    as_i, c_i = run(np.vstack([x, others[:1]]), [g0, og[0]], [o0, oo[0]], k=2)
    as_q, c_q = run(np.vstack([others[:1], x]), [og[0], g0], [oo[0], o0], k=2)
    assert np.array_equal(as_i[0, 0::2], alone[0]) and np.array_equal(c_i[0], c_alone[0])
    assert np.array_equal(as_q[0, 1::2], alone[0]) and np.array_equal(c_q[1], c_alone[0])
    assert np.array_equal(as_i[0, 1::2], as_q[0, 0::2]) and np.array_equal(c_i[1], c_q[0])


def test_side_stream_equals_default_stream():
    n, rows = 4099, 6
    x = rows_input(rows, n, 600)
    g, o = gains_offsets(rows, 16)
    st = distortion.DacStage(g, n, offset=o, interleave=2)
    xd = torch.from_numpy(x).to(dev())
    ca = torch.empty((rows, 3), dtype=torch.int64, device=dev())
    a = st.apply_torch(xd, counts=ca).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z = torch.from_numpy(x).to(dev())
        cb = torch.full((rows, 3), 99, dtype=torch.int64, device=dev())
        b = st.apply_torch(z, counts=cb) + 0                       # produced and consumed on the side stream
        cb = cb + 0
    side.synchronize()
    want, want_counts = ref.dac_ref(x, g, o, interleave=2)
    same(a, want, 'default stream')
    same(b.cpu().numpy(), want, 'side stream')
    same(ca.cpu().numpy(), want_counts, 'default stream, counts')
    same(cb.cpu().numpy(), want_counts, 'side stream, counts')
    st.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_counts_absent(kind):
    n, rows = 8193, 4
    x = rows_input(rows, n, 650, NP_OF[kind])
    g, o = gains_offsets(rows, 12)
    for k in (1, 2):
        st = distortion.DacStage(g, n, offset=o, bits=12, shift=4, interleave=k, dtype=NP_OF[kind])
        assert st.kernel_name() == st.kernel_name(counts=False) == f'dac_rows<{NAME_OF[kind]}>'
        st.close()
        plain, none = run(x, g, o, 12, 4, k, counts=False)
        counted, counts = run(x, g, o, 12, 4, k)
        want, want_counts = ref.dac_ref(x, g, o, 12, 4, k)
        assert none is None
        same(plain, want, f'without counts {kind} k={k}')
        same(counted, want, f'with counts {kind} k={k}')
        same(counts, want_counts, f'counts {kind} k={k}')


def test_overlap_and_refused_tensors():
    n, rows = 256, 4
    st = distortion.DacStage(1000.0, n, batch=rows, interleave=2)
    buf = torch.zeros(rows * n + 64, dtype=torch.float64, device=dev())
    x = buf[:rows * n].view(rows, n)
    as_codes = buf.view(torch.int16)                                      # the same bytes as int16
    out = torch.zeros((2, 2 * n), dtype=torch.int16, device=dev())
    counts = torch.zeros((rows, 3), dtype=torch.int64, device=dev())
    st.apply_torch(x, out, counts)                                        # fine
    for bad_out in (as_codes[:2 * 2 * n].view(2, 2 * n), as_codes[4 * rows * n - 2 * 2 * n + 8:][:2 * 2 * n].view(2, 2 * n)):
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_torch(x, bad_out, counts)
    over_x = buf[8:8 + rows * 3].view(torch.int64).view(rows, 3)
    over_out = out.view(-1)[16:16 + rows * 12].view(torch.int64).view(rows, 3)
    for bad_counts in (over_x, over_out):
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_torch(x, out, bad_counts)
    wide = torch.zeros((rows, 4), dtype=torch.int64, device=dev())
    for bad_counts in (counts[:3], counts.view(-1), wide[:, :3], counts.to(torch.int32), counts.to(torch.float64),
                       counts.cpu(), torch.zeros((rows, 2), dtype=torch.int64, device=dev())):
        with pytest.raises(ValueError, match='counts'):
            st.apply_torch(x, out, bad_counts)
    xc = torch.zeros((rows, n), dtype=torch.float64, device=dev())
    for bad in (xc[:2], xc[:, :n - 1], xc.to(torch.float32), xc.cpu(), xc.t().contiguous().t()):
        with pytest.raises(ValueError):
            st.apply_torch(bad, out)
    for bad in (out[:1], out[:, :2 * n - 1], out.to(torch.int32), out.cpu(), out.t().contiguous().t(),
                torch.zeros((rows, n), dtype=torch.int16, device=dev())):
        with pytest.raises(ValueError):
            st.apply_torch(xc, bad)
    st.close()
    empty = distortion.DacStage([1.0, 2.0], 0, interleave=2)               # n = 0: a no-op that zeroes the counts
    e = torch.zeros((2, 0), dtype=torch.float64, device=dev())
    c = torch.full((2, 3), 5, dtype=torch.int64, device=dev())
    assert tuple(empty.apply_torch(e, counts=c).shape) == (1, 0)
    assert not c.cpu().numpy().any()
    empty.close()


def test_library_refuses_a_bad_apply():
    """the C side's own checks of an apply, through the raw pointers, one case per clause of the row rule: a null
    side, rows not aligned to their element, a stride below the row, overlap, and the report's alignment and overlap
    with either side: WFK_EINVAL, the stage named in the text, nothing launched (the acceptance table itself, the
    lone output row among it: test_row_rule_cpu.py).  n = 0: a no-op that zeroes the report, whatever the row pointers"""
    from waveforms_amd import _engine
    rows, n = 4, 40
    st = distortion.DacStage(1000.0, n, batch=rows)
    x = torch.ones((rows, n), dtype=torch.float64, device=dev())
    out = torch.full((rows, n), SENTINEL, dtype=torch.int16, device=dev())
    counts = torch.full((rows, 3), 7, dtype=torch.int64, device=dev())
    lib, h = _engine.lib(), st.plan._h
    X, Y, C = x.data_ptr(), out.data_ptr(), counts.data_ptr()
    for args, message in (((None, n, Y, n, None), b'null in / out'),
                          ((X, n, None, n, None), b'null in / out'),
                          ((X + 4, n, Y, n, None), b'not aligned to their element'),
                          ((X, n, Y + 1, n, None), b'not aligned to their element'),
                          ((X, n - 1, Y, n, None), b'in row stride smaller'),
                          ((X, n, Y, n - 1, None), b'out row stride smaller'),
                          ((X, n, X + 8, n, None), b'dac rows is out of place: out overlaps in'),
                          ((Y + 2 * rows * n - 8, n, Y, n, None), b'overlaps'),
                          ((X, n, Y, n, C + 4), b'counts are not aligned'),
                          ((X, n, Y, n, X + 16), b'counts overlaps in'),
                          ((X, n, Y, n, Y + 8), b'counts overlaps out')):
        assert lib.wfk_dac_rows_apply(h, *args, None) == -1, args
        text = lib.wfk_last_error()
        assert text.startswith(b'dac rows') and message in text, (args, text)
        with pytest.raises(_engine.EngineError, match=message.decode()):
            st.apply(*args)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL) and np.all(counts.cpu().numpy() == 7)
    st.close()
    empty = distortion.DacStage(1.0, 0, batch=rows)
    assert lib.wfk_dac_rows_apply(empty.plan._h, None, 0, None, 0, C, None) == 0
    torch.cuda.synchronize()
    assert not counts.cpu().numpy().any()
    assert lib.wfk_dac_rows_apply(empty.plan._h, None, 0, None, 0, None, None) == 0
    assert lib.wfk_dac_rows_apply(empty.plan._h, None, 0, None, 0, C + 4, None) == -1
    assert b'counts are not aligned' in lib.wfk_last_error()
    empty.close()


def test_numpy_round_trip():
    rows, n = 6, 3001
    x = rows_input(rows, n, 800)
    g, o = gains_offsets(rows, 14)
    for k in (1, 2):
        want, want_counts = ref.dac_ref(x, g, o, 14, 2, k)
        codes = distortion.dac_codes_rows(x, g, o, bits=14, shift=2, interleave=k)
        same(codes, want, f'dac_codes_rows k={k}')
        codes, counts = distortion.dac_codes_rows(x, g, o, bits=14, shift=2, interleave=k, return_counts=True)
        same(codes, want, f'dac_codes_rows with counts k={k}')
        same(counts, want_counts, f'dac_codes_rows counts k={k}')
    codes, counts = distortion.dac_codes_rows(x.astype(np.float32), 30000.0, return_counts=True)   # scalars: every row
    want, want_counts = ref.dac_ref(x.astype(np.float32), 30000.0)
    same(codes, want, 'float32 rows, one gain')
    same(counts, want_counts, 'float32 rows, one gain, counts')
    xi = (rows_input(rows, 50, 801, specials=False) * 100).astype(np.int32)
    codes = distortion.dac_codes_rows(xi, 1.0, offset=0.5)                                         # read as float64
    same(codes, ref.dac_ref(xi.astype(np.float64), 1.0, 0.5)[0], 'integer input')


def test_loop_back_through_the_demodulator():
    """two-tone shots sampled on the device, quantised by the stage, demodulated from the int16 codes, against the
    float64 traces demodulated directly.  A code is within 0.5 LSB of v = x gain, and the default weights 2 / N sum
    to 2 in magnitude over the N points: |iq_codes / gain - iq_float| <= 2 * 0.5 / gain, plus 1e-9 * scale for the
    two float64 sums."""
    from waveforms_amd import cos
    from waveforms_amd._sampling import BatchSampler
    from waveforms_amd.utils import Demodulator
    shots, n, fs = 10, 4096, [50e6, 125e6]
    ro = [0.2 * cos(2 * np.pi * 50e6, 0.1 * s) + 0.1 * cos(2 * np.pi * 125e6) for s in range(shots)]
    traces = BatchSampler(ro, ('linspace', 0.0, 4096e-9, n, False)).launch_torch(
        torch.empty((shots, n), dtype=torch.float64, device=dev()))
    full_scale = 0.35
    st = distortion.DacStage.from_full_scale(full_scale, n, batch=shots)
    gain = st.hi / full_scale
    assert np.all(st.gain == gain)
    counts = torch.empty((shots, 3), dtype=torch.int64, device=dev())
    codes = st.apply_torch(traces, counts=counts)
    assert not counts.cpu().numpy().any()
    iq_codes = Demodulator(fs, n, dtype=np.int16).apply_torch(codes).cpu().numpy()
    iq_float = Demodulator(fs, n, dtype=np.float64).apply_torch(traces).cpu().numpy()
    scale = float(traces.abs().max())
    err = np.abs(iq_codes / gain - iq_float)
    print(f'loop-back: max |iq_codes / gain - iq_float| = {err.max():.3g}, bound {1 / gain + 1e-9 * scale:.3g}')
    assert iq_codes.shape == (shots, 2) and np.all(err <= 1 / gain + 1e-9 * scale)
    assert np.all(np.abs(np.abs(iq_float) - [0.2, 0.1]) < 1e-3)
    st.close()


def test_plain_c_consumer_quantises_on_the_device(tmp_path):
    exe = tmp_path / 'dac_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'dac_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'quantised on the device, parity ok' in r.stdout, r.stdout
