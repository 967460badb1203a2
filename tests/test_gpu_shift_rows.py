"""Per-row shift on the device (distortion.ShiftStage / shift_rows, csrc/wfk_shift_rows.hip) against the referee
tests/shift_rows_ref.py, the closed form of the reference's shift(signal, delay, dt).

Bound, per element: 4 * 2^-53 * B_i for float64 rows, B_i = |1 - d| |x[i - p]| + |d| |x[i - p - 1]| (two rounded products
and one rounded sum on each side), plus 2^-24 * |y_ref| for float32 rows (computed in float64, rounded once on the
store); exactly zero where the result is zero fill.  Whole-sample delays move bits and are compared as bits."""
import os
import subprocess

import numpy as np
import pytest
import torch

import shift_rows_ref as ref
from waveforms_amd import distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 4099, 10007]
DELTAS = [0.0, 0.25, 2.0**-40, 1.0]
NP_OF = {'f64': np.float64, 'f32': np.float32}


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def points_of(n):
    """every alignment class of source against destination for 8-B and 4-B elements, both ends, rows pushed out"""
    return [0, 1, -1, 2, -2, 3, -3, n - 1, -(n - 1), n, -n, n + 5, -(n + 5)]


def rows_input(rows, n, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(rows, n)) * np.exp(rng.uniform(-3, 3, (rows, n)))).astype(dtype)


def run_split(x, points, deltas):
    """x (rows, n) NumPy of the stage's dtype -> the stage's result for rows split as (points, deltas)"""
    st = distortion.ShiftStage.from_split(points, deltas, x.shape[1], x.dtype)
    try:
        out = torch.full(x.shape, 9.0, dtype=torch.from_numpy(x).dtype, device=dev())
        return st.apply_torch(torch.from_numpy(x).to(dev()), out).cpu().numpy()
    finally:
        st.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', SIZES)
def test_small_shapes(n, kind):
    dtype = NP_OF[kind]
    pd = [(p, d) for p in points_of(n) for d in DELTAS]
    points, deltas = [p for p, _ in pd], [d for _, d in pd]
    x = rows_input(len(pd), n, 100 + n, dtype)
    st = distortion.ShiftStage.from_split(points, deltas, n, dtype)
    assert st.kernel_name() == ('shift_rows<double>' if kind == 'f64' else 'shift_rows<float>')
    assert list(st.points) == points and list(st.deltas) == deltas
    st.close()
    got = run_split(x, points, deltas)
    assert got.dtype == dtype
    want, B = ref.shift_rows_ref(x, points, deltas)
    ref.check(got, want, B, f'n={n} {kind}', ref.EPS32 if kind == 'f32' else 0.0)
    if kind == 'f64':
        for r, (p, d) in enumerate(pd):
            if abs(p) >= n:
                assert not got[r].any()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_whole_sample_delays_move_bits(kind):
    """delta = 0: no arithmetic, the zero-filled integer shift of the bits, +-inf and NaN included"""
    dtype = NP_OF[kind]
    for n in (5, 257, 4099):
        points = points_of(n) + [17, -64, 128]
        x = rows_input(len(points), n, 300 + n, dtype)
        x[:, ::7] = np.inf
        x[:, 1::11] = -np.inf
        x[:, 2::13] = np.nan
        x[:, 3::17] = -0.0
        got = run_split(x, points, [0.0] * len(points))
        want = np.zeros_like(x)
        for r, p in enumerate(points):
            if 0 <= p < n:
                want[r, p:] = x[r, :n - p]
            elif -n < p < 0:
                want[r, :n + p] = x[r, -p:]
        assert np.array_equal(bits(got), bits(want)), (n, kind)


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', [5, 4099])
def test_windows_and_canaries(n, kind):
    """row stride n + 37, rows that start 40 B into a buffer, a strided out: nothing outside a row of `out` is
    written, the input is intact"""
    dtype = NP_OF[kind]
    tdt = torch.float64 if kind == 'f64' else torch.float32
    off = 40 // np.dtype(dtype).itemsize
    delays = [0.0, 0.3, -1.25, 2.5, -(n - 0.5), 3.0, n + 2.0]
    rows = len(delays)
    x = rows_input(rows, n, 400 + n, dtype)
    st = distortion.ShiftStage(delays, n, 1.0, dtype)
    want, B = ref.shift_rows_ref(x, st.points, st.deltas)
    eps = ref.EPS32 if kind == 'f32' else 0.0
    wide = torch.full((rows, n + 37), 7.0, dtype=tdt, device=dev())
    win = wide[:, off:off + n]
    win.copy_(torch.from_numpy(x))
    for lead in (0, 1, 2, 3, 5):                          # the output rows start at every offset into a 16-B slot
        out = torch.full((rows, n + 64), -3.0, dtype=tdt, device=dev())
        res = st.apply_torch(win, out[:, lead:lead + n])
        assert res.data_ptr() == out[:, lead:].data_ptr()
        o = out.cpu().numpy()
        ref.check(o[:, lead:lead + n], want, B, f'window n={n} {kind} lead={lead}', eps)
        assert np.all(o[:, :lead] == -3.0) and np.all(o[:, lead + n:] == -3.0)
    w = wide.cpu().numpy()
    assert np.array_equal(w[:, off:off + n], x) and np.all(w[:, :off] == 7.0) and np.all(w[:, off + n:] == 7.0)
    # a contiguous input into a window of the wide buffer
    xc = torch.from_numpy(x).to(dev())
    wide2 = torch.full((rows, n + 37), 7.0, dtype=tdt, device=dev())
    st.apply_torch(xc, wide2[:, off:off + n])
    w = wide2.cpu().numpy()
    ref.check(w[:, off:off + n], want, B, f'into a window n={n} {kind}', eps)
    assert np.all(w[:, :off] == 7.0) and np.all(w[:, off + n:] == 7.0)
    st.close()


@pytest.mark.parametrize('n', [257, 10007])
def test_row_independence(n):
    """a row's result is bitwise the same alone, first and last in a batch whose other rows differ"""
    x = rows_input(1, n, 500 + n)
    others = rows_input(4, n, 501 + n)
    op, od = [3, -n, 0, -7], [0.0, 0.5, 1.0, 0.125]
    for p, d in ((5, 0.3), (-3, 2.0**-40), (0, 0.0)):
        alone = run_split(x, [p], [d])[0]
        first = run_split(np.vstack([x, others]), [p] + op, [d] + od)[0]
        last = run_split(np.vstack([others, x]), op + [p], od + [d])[4]
        assert np.array_equal(bits(alone), bits(first)) and np.array_equal(bits(alone), bits(last))
        want, B = ref.shift_ref(x[0], p, d)
        ref.check(alone, want, B, f'alone n={n} p={p} d={d}')


def test_side_stream_equals_default_stream():
    n, rows = 4099, 6
    x = rows_input(rows, n, 600)
    st = distortion.ShiftStage([0.3, -2.75, 5.0, 0.0, -(n + 1.0), 1000.5], n, 1.0)
    xd = torch.from_numpy(x).to(dev())
    a = st.apply_torch(xd, torch.empty_like(xd)).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z = torch.from_numpy(x).to(dev())
        b = st.apply_torch(z, torch.empty_like(z)) * 1.0          # produced and consumed on the side stream
    side.synchronize()
    assert np.array_equal(bits(a), bits(b.cpu().numpy()))
    want, B = ref.shift_rows_ref(x, st.points, st.deltas)
    ref.check(a, want, B, 'streams')
    st.close()


def test_many_workgroups_per_row():
    rows, n = 64, 100003
    rng = np.random.default_rng(700)
    x = rows_input(rows, n, 701)
    delays = rng.uniform(-3000.0, 3000.0, rows)
    delays[:6] = [0.0, 17.0, -4096.0, n - 0.5, -(n - 0.25), n + 1.0]
    st = distortion.ShiftStage(delays, n, 1.0)
    xd = torch.from_numpy(x).to(dev())
    got = st.apply_torch(xd, torch.empty_like(xd)).cpu().numpy()
    want, B = ref.shift_rows_ref(x, st.points, st.deltas)
    ref.check(got, want, B, f'{rows} x {n}')
    st.close()


def test_against_the_single_signal_shift():
    """shift_rows agrees with distortion.shift (upload, 3-tap FIR, download, host shift) row by row within the
    1e-12 * scale that function is held to"""
    n, fs = 3001, 2e9
    x = rows_input(5, n, 800)
    delays = [3.3 / fs, -3.3 / fs, 0.0, 12.0 / fs, -250.75 / fs]
    got = distortion.shift_rows(x, delays, 1 / fs)
    assert got.dtype == np.float64 and got.shape == x.shape
    for r, d in enumerate(delays):
        scale = max(1.0, float(np.abs(x[r]).max()))
        assert np.max(np.abs(got[r] - distortion.shift(x[r], d, 1 / fs))) <= 1e-12 * scale, r
    points, deltas = zip(*[ref.split(d, 1 / fs) for d in delays])
    want, B = ref.shift_rows_ref(x, points, deltas)
    ref.check(got, want, B, 'shift_rows')
    same = distortion.shift_rows(x, 3.3 / fs, 1 / fs)                      # a scalar: every row
    want, B = ref.shift_rows_ref(x, [3] * 5, [ref.split(3.3 / fs, 1 / fs)[1]] * 5)
    ref.check(same, want, B, 'shift_rows, one delay')
    x32 = x.astype(np.float32)
    got32 = distortion.shift_rows(x32, delays, 1 / fs)
    assert got32.dtype == np.float32
    want, B = ref.shift_rows_ref(x32, points, deltas)
    ref.check(got32, want, B, 'shift_rows float32', ref.EPS32)
    # 1.0 // 0.1 = 9 and delta = 1: legal
    got = distortion.shift_rows(x[:1], 1.0, 0.1)
    want, B = ref.shift_ref(x[0], 9, 1.0)
    ref.check(got[0], want, B, 'delta = 1')


def test_overlap_and_refused_tensors():
    n, rows = 256, 3
    st = distortion.ShiftStage(0.5, n, 1.0, batch=rows)
    buf = torch.zeros((2 * rows, n + 8), dtype=torch.float64, device=dev())
    x, y = buf[:rows, :n], buf[rows:, :n]
    st.apply_torch(x, y)                                                  # disjoint rows of one buffer: fine
    for out in (x, buf[1:rows + 1, :n], buf[:rows, 4:4 + n], buf[rows - 1:2 * rows - 1, 8:8 + n]):
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_torch(x, out)
    xc = torch.zeros((rows, n), dtype=torch.float64, device=dev())
    ok = torch.empty_like(xc)
    for bad in (xc[:2], xc[:, :n - 1], xc.to(torch.float32), xc.cpu(), xc.t().contiguous().t()):
        with pytest.raises(ValueError):
            st.apply_torch(bad, ok)
        with pytest.raises(ValueError):
            st.apply_torch(xc, bad)
    st.close()
    empty = distortion.ShiftStage([0.5, -1.0], 0, 1.0)                    # n = 0: a no-op
    e = torch.zeros((2, 0), dtype=torch.float64, device=dev())
    assert empty.apply_torch(e, torch.zeros_like(e)).shape == (2, 0)
    empty.close()


def test_plain_c_consumer_shifts_on_the_device(tmp_path):
    exe = tmp_path / 'shift_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'shift_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'shifted on the device, parity ok' in r.stdout, r.stdout
