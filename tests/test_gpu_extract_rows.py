"""Per-row kernel extraction on the device (distortion.KernelExtractor / extract_kernel_rows,
csrc/wfk_extract_rows.hip) against the referee tests/extract_rows_ref.py.

Bound, per row: max(1e-12 * scale, 10 * self_err) against the referee's long-double result (scale = its max, self_err
= its distance from the referee's own float64 leg); the referee asserts self_err <= 1e-13 * scale for every case, so
the floor governs and the second term hides nothing.

Inputs: row r of size n is the recipe of tests/cases.extract_input with the seed SEEDS[n][r], sig_out scaled by
10^(r mod 3).  SEEDS[n][r] is the first seed s >= n + 1000 r at which the referee's two legs agree to 0.5e-13 * scale
at every M and every skip of the grid below -- a property of the referee alone (no device result enters it), needed
because skip = n // 2 leaves ONE sample of an odd row, c[n - 1], which is 1e-2 .. 1e-5 of the row's peak, and the
transforms' error is relative to the peak: at seed n itself that sample sits at 2e-13 (n = 1023, M = 4) and 3.9e-13
(n = 4099, no taps) of its own size between the two legs.  The shared sig_in of size n and its image take
SHARED_SEEDS[n], the first seed s >= n that passes the same rule for all five scaled rows (the scale factors are no
powers of two, so every row rounds on its own: at seed 4102 row 3 sits at 1.3e-13).  No (n, M, skip) is left out."""
import os
import subprocess

import numpy as np
import pytest
import torch

import extract_rows_ref as ref
from waveforms_amd import distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 2e9
SIZES = [1, 2, 3, 4, 5, 16, 255, 256, 257, 1023, 4099, 10007]
BIG_M = 1500          # more than extract_smooth's LDS halo (kTapBlock = 1024 taps per pass)
SEEDS = {1: [1, 1001, 2001, 3001, 4001], 2: [2, 1002, 2002, 3002, 4002], 3: [3, 1003, 2003, 3003, 4003],
         4: [4, 1004, 2004, 3004, 4004], 5: [5, 1005, 2005, 3005, 4005], 16: [16, 1016, 2016, 3016, 4016],
         255: [255, 1255, 2255, 3255, 4255], 256: [256, 1256, 2256, 3256, 4256], 257: [257, 1258, 2257, 3257, 4259],
         1023: [1024, 2023, 3023, 4023, 5023], 4099: [4102, 5099, 6099, 7100, 8101],
         10007: [10007, 11011, 12015, 13017, 14008]}
SHARED_SEEDS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 16: 16, 255: 255, 256: 256, 257: 257, 1023: 1024, 4099: 4104,
                10007: 10013}


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def taps_list(n):
    Ms = [None] + [M for M in (4, 5, 10, 36, 37, n) if 4 <= M <= n] + ([BIG_M] if n == 10007 else [])
    return list(dict.fromkeys(Ms))


def skips_of(n):
    return list(dict.fromkeys([0, 1, 3, n // 2, n // 2 + 1]))


def bw_of(M):
    return None if M is None else ref.bw_for(M, FS)


def rows_input(n, rows=5, seeds=None):
    """(a, b): (rows, n) each; sig_out row r scaled by 10^(r mod 3)"""
    ab = [ref.make_input(n, s) for s in (seeds or SEEDS[n][:rows])]
    return np.stack([a for a, _ in ab]), np.stack([b * 10.0**(r % 3) for r, (_, b) in enumerate(ab)])


def shared_input(n, rows=5):
    """one sig_in and its image, the rows scaled apart: 10^(r mod 3) * (1 + r / 4)"""
    a, b = ref.make_input(n, SHARED_SEEDS[n])
    return a, np.stack([b * (10.0**(r % 3) * (1 + r / 4)) for r in range(rows)])


def run(a, b, bw=None, skip=0, out=None):
    """NumPy rows -> the stage's result as NumPy; a 1-D: shared"""
    ex = distortion.KernelExtractor(b.shape[1], b.shape[0], FS, bw, skip, shared_input=a.ndim == 1)
    try:
        got = ex.apply_torch(torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev()), out)
        assert got.shape == (b.shape[0], ex.k)
        return got.cpu().numpy()
    finally:
        ex.close()


@pytest.mark.parametrize('shared', [False, True], ids=['per_row', 'shared'])
@pytest.mark.parametrize('n', SIZES)
def test_parity(n, shared):
    a, b = shared_input(n) if shared else rows_input(n)
    case = 0
    for M in taps_list(n):
        full = ref.rows_ref(a, b, ref.taps_of(FS, bw_of(M)), 0, (n, M))
        for skip in skips_of(n):
            rows = 1 + case % 5                                   # batches of 1 .. 5 rows
            case += 1
            got = run(a if shared else a[:rows], b[:rows], bw_of(M), skip)
            want = full.crop(skip, rows, (n, M, skip))
            assert got.shape == want.want.shape == (rows, max(n - 2 * skip, 0))
            want.check(got, f'n={n} M={M} skip={skip} rows={rows} shared={shared}')
    ex = distortion.KernelExtractor(n, 2, FS, bw_of(taps_list(n)[-1]), 1)
    assert ex.kernel_name() == 'extract_ratio + extract_smooth'
    assert (ex.n, ex.batch, ex.k) == (n, 2, max(n - 2, 0))
    M = taps_list(n)[-1]
    assert (ex.taps is None) if M is None else np.array_equal(ex.taps, ref.taps_of(FS, bw_of(M)))
    ex.close()


@pytest.mark.parametrize('n', [5, 256, 4099])
def test_no_taps_moves_bits(n):
    """without taps the last pass is rotation + crop: any skip equals the crop of the stage's own skip = 0 result"""
    a, b = rows_input(n, 3)
    for bw in (None, FS, 0.5 * FS):                               # bw >= sample_rate / 2: the reference does not smooth
        whole = run(a, b, bw, 0)
        for skip in skips_of(n):
            got = run(a, b, bw, skip)
            assert np.array_equal(bits(got), bits(whole[:, skip:max(n - skip, skip)])), (n, bw, skip)


@pytest.mark.parametrize('M', [None, 10])
@pytest.mark.parametrize('n', [5, 4099])
def test_windows_and_canaries(n, M):
    """inputs of row stride n + 37 at 8-byte and 40-byte row offsets, output rows of stride K + 5 at every offset of
    a row into a 16-byte slot: nothing outside a result row is written, the inputs are intact"""
    if M is not None and M > n:
        M = 4
    rows, skip = 3, 1
    K = n - 2 * skip
    a, b = rows_input(n, rows)
    want = ref.rows_ref(a, b, ref.taps_of(FS, bw_of(M)), skip, (n, M))
    ex = distortion.KernelExtractor(n, rows, FS, bw_of(M), skip)
    wa = torch.full((rows, n + 37), 7.0, dtype=torch.float64, device=dev())
    wb = torch.full((rows, n + 37), 7.0, dtype=torch.float64, device=dev())
    for off in (1, 5):
        wa[:, off:off + n].copy_(torch.from_numpy(a))
        wb[:, off:off + n].copy_(torch.from_numpy(b))
        for lead in (0, 1, 2, 3):                                 # K + 5 odd or even: rows start on both slot halves
            buf = torch.full((rows * (K + 5) + 8,), -3.0, dtype=torch.float64, device=dev())
            out = buf[lead:lead + rows * (K + 5)].view(rows, K + 5)[:, :K]
            res = ex.apply_torch(wa[:, off:off + n], wb[:, off:off + n], out)
            assert res.data_ptr() == out.data_ptr() and res.shape == (rows, K)
            o = buf.cpu().numpy()
            body = o[lead:lead + rows * (K + 5)].reshape(rows, K + 5)
            want.check(np.ascontiguousarray(body[:, :K]), f'window n={n} M={M} off={off} lead={lead}')
            assert np.all(o[:lead] == -3.0) and np.all(body[:, K:] == -3.0) and np.all(o[lead + rows * (K + 5):] == -3.0)
        for w, x in ((wa, a), (wb, b)):
            h = w.cpu().numpy()
            assert np.array_equal(h[:, off:off + n], x)
            h[:, off:off + n] = 7.0
            assert np.all(h == 7.0)
            w.fill_(7.0)
    ex.close()


@pytest.mark.parametrize('M', [None, 36])
def test_side_stream_and_second_apply(M):
    n, rows, skip = 4099, 4, 3
    a, b = rows_input(n, rows)
    a2, b2 = rows_input(n, rows, [n + 50000 + r for r in range(rows)])
    ex = distortion.KernelExtractor(n, rows, FS, bw_of(M), skip)
    ad, bd = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
    first = ex.apply_torch(ad, bd).cpu().numpy()
    ref.rows_ref(a, b, ex.taps, skip, 'first').check(first, f'first apply M={M}')
    second = ex.apply_torch(torch.from_numpy(a2).to(dev()), torch.from_numpy(b2).to(dev())).cpu().numpy()
    ref.rows_ref(a2, b2, ex.taps, skip, 'second').check(second, f'second apply, other data M={M}')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        az, bz = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
        third = ex.apply_torch(az, bz) * 1.0                      # produced and consumed on the side stream
    side.synchronize()
    assert np.array_equal(bits(first), bits(third.cpu().numpy()))
    ex.close()


@pytest.mark.parametrize('n', [257, 10007])
def test_row_independence(n):
    """row r alone, first and last of a batch: each within the bound (rocFFT may choose another plan per batch size,
    so equality as bits is not asserted)"""
    a, b = rows_input(n, 5)
    for M in (None, 10):
        one = ref.rows_ref(a[:1], b[:1], ref.taps_of(FS, bw_of(M)), 1, (n, M))
        alone = run(a[:1], b[:1], bw_of(M), 1)
        first = run(a, b, bw_of(M), 1)[:1]
        order = [1, 2, 3, 4, 0]
        last = run(a[order], b[order], bw_of(M), 1)[4:]
        for got, what in ((alone, 'alone'), (first, 'first'), (last, 'last')):
            one.check(got, f'n={n} M={M} {what}')


@pytest.mark.parametrize('shared', [False, True], ids=['per_row', 'shared'])
def test_zero_row_of_sig_out(shared):
    """an all-zero sig_out row: every bin divides by zero, the row is not finite; its neighbours are within the bound"""
    n, skip = 1023, 3
    a, b = shared_input(n, 4) if shared else rows_input(n, 4)
    b[2] = 0.0
    for M in (None, 10):
        got = run(a, b, bw_of(M), skip)
        assert not np.any(np.isfinite(got[2])), (M, got[2])
        keep = [0, 1, 3]
        want = ref.rows_ref(a if shared else a[keep], b[keep], ref.taps_of(FS, bw_of(M)), skip, (n, M))
        want.check(np.ascontiguousarray(got[keep]), f'neighbours of a zero row M={M} shared={shared}')


def test_overlap_and_refused_tensors():
    n, rows, skip = 256, 3, 2
    K = n - 2 * skip
    ex = distortion.KernelExtractor(n, rows, FS, None, skip)
    buf = torch.ones((3 * rows, n + 8), dtype=torch.float64, device=dev())
    a, b, y = buf[:rows, :n], buf[rows:2 * rows, :n], buf[2 * rows:, :K]
    assert ex.apply_torch(a, b, y).data_ptr() == y.data_ptr()          # disjoint rows of one buffer: fine
    ex.apply_torch(a, a, y)                                            # the inputs may be the same rows
    ex.apply_torch(a, buf[1:rows + 1, 4:4 + n], y)                     # ... or overlap
    for out in (a[:, :K], b[:, :K], buf[1:rows + 1, :K], buf[rows - 1:2 * rows - 1, 8:8 + K], buf[2 * rows - 1:-1, :K]):
        with pytest.raises(ValueError, match='overlaps'):
            ex.apply_torch(a, b, out)
    ok = torch.ones((rows, n), dtype=torch.float64, device=dev())
    for bad in (ok[:2], ok[:, :n - 1], ok.to(torch.float32), ok.cpu(), ok.t().contiguous().t(), ok[0]):
        with pytest.raises(ValueError):
            ex.apply_torch(bad, ok)
        with pytest.raises(ValueError):
            ex.apply_torch(ok, bad)
    for bad in (torch.ones((rows, K - 1), dtype=torch.float64, device=dev()), torch.ones((rows, K)),
                torch.ones((rows - 1, K), dtype=torch.float64, device=dev())):
        with pytest.raises(ValueError):
            ex.apply_torch(ok, ok.clone(), bad)
    ex.close()
    sh = distortion.KernelExtractor(n, rows, FS, None, skip, shared_input=True)
    one = sh.apply_torch(ok[0], ok)                                    # 1-D and (1, n) are the same thing
    two = sh.apply_torch(ok[:1], ok)
    assert np.array_equal(bits(one.cpu().numpy()), bits(two.cpu().numpy()))
    with pytest.raises(ValueError):
        sh.apply_torch(ok, ok)
    sh.close()
    empty = distortion.KernelExtractor(n, rows, FS, None, n // 2)      # K = 0: a no-op
    assert empty.k == 0 and empty.apply_torch(ok, ok).shape == (rows, 0)
    empty.close()


def test_library_refuses_a_bad_apply():
    """the C side's own checks of an apply, through the raw pointers, one case per clause of the row rule with two
    inputs against one result: a null side, rows not aligned to their element, a stride below the row on each side,
    the result meeting either input: WFK_EINVAL, the stage named in the text, nothing launched"""
    from waveforms_amd import _engine
    rows, n, skip = 4, 40, 3
    K = n - 2 * skip
    ex = distortion.KernelExtractor(n, rows, FS, None, skip)
    a = torch.ones((rows, n), dtype=torch.float64, device=dev())
    b = torch.ones((rows, n), dtype=torch.float64, device=dev())
    y = torch.full((rows, K), -7.0, dtype=torch.float64, device=dev())
    lib, h = _engine.lib(), ex.plan._h
    A, B, Y = a.data_ptr(), b.data_ptr(), y.data_ptr()
    for args, message in (((None, n, B, n, Y, K), b'null'),
                          ((A, n, None, n, Y, K), b'null'),
                          ((A, n, B, n, None, K), b'null'),
                          ((A + 4, n, B, n, Y, K), b'not aligned'),
                          ((A, n, B + 4, n, Y, K), b'not aligned'),
                          ((A, n, B, n, Y + 4, K), b'not aligned'),
                          ((A, n - 1, B, n, Y, K), b'sig_in row stride smaller'),
                          ((A, n, B, n - 1, Y, K), b'sig_out row stride smaller'),
                          ((A, n, B, n, Y, K - 1), b'ker row stride smaller'),
                          ((A, n, B, n, A + 8 * (rows * n - 1), K), b'ker overlaps sig_in'),
                          ((A, n, B, n, B + 8, K), b'ker overlaps sig_out'),
                          ((Y + 8 * (rows * K - 1), n, B, n, Y, K), b'ker overlaps sig_in')):
        assert lib.wfk_extract_rows_apply(h, *args, None) == -1, args
        text = lib.wfk_last_error()
        assert text.startswith(b'extract rows') and message in text, (args, text)
        with pytest.raises(_engine.EngineError, match=message.decode()):
            ex.apply(*args)
    torch.cuda.synchronize()
    assert np.all(y.cpu().numpy() == -7.0)
    ex.close()


def test_many_workgroups_per_row():
    """64 x 100 003, M = 40: 49 workgroups per row in extract_smooth, 25 in extract_ratio.  The long-double transform
    of a row of this (prime) length takes 0.4 s on the host, so the 64 rows are 8 pairs of signals (seeds n + 1000 p),
    row r the pair r mod 8 with sig_out times 2^(r // 8 - 3): a power of two scales every step of both legs exactly,
    so the referee of row r is the referee of its pair times 2^(3 - r // 8), and every row is held to its own bound."""
    rows, n, M, skip, pairs = 64, 100003, 40, 2, 8
    a8, b8 = rows_input(n, pairs, [n + 1000 * p for p in range(pairs)])
    base = ref.rows_ref(a8, b8, ref.taps_of(FS, ref.bw_for(M, FS)), skip, 'big')
    power = np.array([2.0**(r // pairs - 3) for r in range(rows)])
    which = np.arange(rows) % pairs
    a, b = a8[which], b8[which] * power[:, None]
    got = distortion.extract_kernel_rows(a, b, FS, ref.bw_for(M, FS), skip)
    want = ref.Ref(base.want[which] / power[:, None].astype(np.longdouble), base.f64[which] / power[:, None])
    want.assert_conditioned('big')
    want.check(got, f'{rows} x {n} M={M}')


def test_numpy_wrapper_shared_and_per_row():
    n = 1023
    a, b = rows_input(n, 3)
    ref.rows_ref(a, b, ref.taps_of(FS, 0.2e9), 5, 'wrapper').check(
        distortion.extract_kernel_rows(a, b, FS, 0.2e9, 5), 'extract_kernel_rows')
    a1, b1 = shared_input(n, 3)
    ref.rows_ref(a1, b1, None, 0, 'wrapper shared').check(distortion.extract_kernel_rows(a1, b1, FS),
                                                          'extract_kernel_rows, shared')


def test_loop_closure_through_fir_stage():
    """three rows distorted by FirStage with three known short kernels; the extracted kernels (K = 1025) restore them
    through FirStage as the kernels of host distortion.extractKernel do: this holds the stage against the host
    function it replaces, not the deconvolution's own truncation error.  Bound: the referee's relative bound of the
    row's kernel, max(1e-12, 10 * self_err / scale), times sum |ker| times max |distorted row|."""
    n, rows, K = 4097, 3, 1025
    skip = (n - K) // 2
    x = np.stack([ref.make_input(n, 900 + r)[0] for r in range(rows)])
    short = np.zeros((rows, 49))
    for r in range(rows):                                              # causal, minimum phase: 0.3 delta + a decay
        k = np.exp(-np.arange(25) / (4.0 + r))
        short[r, 24:] = k / k.sum()
        short[r, 24] += 0.3
    xd = torch.from_numpy(x).to(dev())
    fwd = distortion.FirStage(short, n, rows)
    y = fwd.apply_torch(xd, torch.empty_like(xd))
    fwd.close()
    yh = y.cpu().numpy()
    ex = distortion.KernelExtractor(n, rows, FS, None, skip)
    assert ex.k == K
    ker_dev = ex.apply_torch(xd, y).cpu().numpy()
    ex.close()
    want = ref.rows_ref(x, yh, None, skip, 'loop')
    want.check(ker_dev, 'loop closure: extracted kernels')
    ker_host = np.stack([distortion.extractKernel(x[r], yh[r], FS, None, skip) for r in range(rows)])
    restored = []
    for ker in (ker_dev, ker_host):
        back = distortion.FirStage(ker, n, rows)
        restored.append(back.apply_torch(y, torch.empty_like(y)).cpu().numpy())
        back.close()
    for r in range(rows):
        tol = want.bound[r] / want.scale[r] * np.sum(np.abs(ker_host[r])) * np.max(np.abs(yh[r]))
        err = float(np.max(np.abs(restored[0][r] - restored[1][r])))
        print(f'row {r}: restored rows differ by {err:.3g}, bound {tol:.3g}; from x by '
              f'{float(np.max(np.abs(restored[0][r][K:-K] - x[r][K:-K]))):.3g} inside')
        assert err <= tol, (r, err, tol)


def test_plain_c_consumer_extracts_on_the_device(tmp_path):
    exe = tmp_path / 'extract_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'extract_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'kernels extracted on the device, parity ok' in r.stdout, r.stdout
