"""The mix stage on the device (distortion.MixStage / mix_rows, csrc/wfk_mix_rows.hip) against the referee
tests/mix_rows_ref.py, the NumPy statement of the semantics.  The formula rounds every product and every sum in
float64, in ascending column order, as the NumPy loop does: every comparison here is exact -- the bits are equal
wherever the referee is not NaN, and NaN stands exactly where the referee has NaN.  There is no tolerance."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import dac_rows_ref
import mix_rows_ref as ref
from row_windows import FarWindow, Window, free_far_arena
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _engine.MIX_TILE_ROWS
NP_OF = {'f64': np.float64, 'f32': np.float32}
NAME_OF = {'f64': 'double', 'f32': 'float'}
SPAN = {'f64': 2048, 'f32': 4096}                        # kSlots * kThreads * V samples: one workgroup's span
SENTINEL = {'f64': -1.2345e300, 'f32': -1.2345e30}


def sizes(kind):
    s = SPAN[kind]
    return [1, 2, 3, 7, 8, 9, 1023, 1024, 1025, s - 1, s, s + 1, 10007]


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def shapes():
    """(name, matrix, offset or None): every shape of the file's small-shape test"""
    rng = np.random.default_rng(11)
    blocks, iq_off = ref.iq_blocks(3, 12)
    hole = ref.band(3 * T, 1, 13)
    hole[T:2 * T] = 0.0
    out = [('1x1', np.array([[-1.75]]), [0.5]),
           ('permutation-5', ref.permutation(5, 14)[0], None),
           ('iq-6', ref.block_diagonal(blocks), iq_off)]
    out += [(f'tridiagonal-{r}', ref.band(r, 1, 15 + r), rng.uniform(-1, 1, r)) for r in (T - 1, T, T + 1, 2 * T + 1)]
    out += [('dense-19x17', ref.dense(19, 17, 16), rng.uniform(-1, 1, 19))]
    out += [(f'long-row-{k}', ref.one_long_row(T + 3, k, 5, 17 + k), None) for k in (9, 17, 40)]
    out += [('empty-tile', hole, rng.uniform(-1, 1, 3 * T)),
            ('3x11', ref.dense(3, 11, 18) * (rng.uniform(size=(3, 11)) < 0.6), [0.0, -0.0, 1.0]),
            ('11x3', ref.dense(11, 3, 19) * (rng.uniform(size=(11, 3)) < 0.6), None)]
    return out


SHAPES = shapes()


def run(x, matrix, offset=None):
    """x (rows_in, n) NumPy -> the (rows_out, n) result of a stage built for it, from contiguous tensors, the output
    allocated by the stage"""
    st = distortion.MixStage(matrix, x.shape[1], offset=offset, dtype=x.dtype)
    try:
        y = st.apply_torch(torch.from_numpy(x).to(dev()))
        assert tuple(y.shape) == (st.rows_out, x.shape[1]) and y.is_contiguous()
        return y.cpu().numpy()
    finally:
        st.close()


def test_the_shapes_are_what_they_are_named():
    by = {name: m for name, m, _ in SHAPES}
    assert ref.reads_of(by['dense-19x17'], T) == 3 * 17 and by['dense-19x17'].shape[0] % T == 3      # three chunks, partial tile
    for k in (9, 17, 40):
        m = by[f'long-row-{k}']
        assert np.count_nonzero(m[5]) == k and sorted(np.count_nonzero(m, axis=1))[:-1] == [1] * (T + 2)
    assert not by['empty-tile'][T:2 * T].any() and by['empty-tile'][:T].any() and by['empty-tile'][2 * T:].any()
    assert by['3x11'].shape == (3, 11) and by['11x3'].shape == (11, 3)
    assert 0 < np.count_nonzero(by['3x11']) < 33 and 0 < np.count_nonzero(by['11x3']) < 33


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('index', range(13))
def test_small_shapes(index, kind):
    n = sizes(kind)[index]
    for name, m, off in SHAPES:
        x = ref.rows_input(m.shape[1], n, 100 + n, NP_OF[kind])
        ref.same_bits(run(x, m, off), ref.mix_ref(x, m, off), f'{name} n={n} {kind}')


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_special_values(kind):
    """a NaN-filled input row reaches exactly the outputs that have a term on it; coefficients that overflow float32"""
    n = 1025
    x = ref.rows_input(2 * T + 1, n, 7, NP_OF[kind], specials=False)
    x[T - 1] = np.nan                                    # the band couples it to rows T - 2, T - 1, T: two tiles
    m = ref.band(2 * T + 1, 1, 8)
    y = run(x, m)
    ref.same_bits(y, ref.mix_ref(x, m), f'NaN row {kind}')
    nan_rows = np.isnan(y).all(axis=1)
    assert nan_rows.tolist() == [T - 2 <= o <= T for o in range(2 * T + 1)] and not np.isnan(y[~nan_rows]).any()
    big = ref.band(T + 1, 1, 9) * (1e300 if kind == 'f64' else 1e39)       # float32: |x| > 0.34 on the diagonal overflows
    y = run(x[:T + 1], big, np.full(T + 1, 1.0))
    want = ref.mix_ref(x[:T + 1], big, np.full(T + 1, 1.0))
    ref.same_bits(y, want, f'overflow {kind}')
    if kind == 'f32':
        assert np.isinf(want[:T - 2]).sum() > 100 and np.isfinite(want[:T - 2]).sum() > 100


def test_order_and_contraction_sensitive_rows():
    """rows on which another summation order or a fused multiply-add changes the bits of every sample
    (tests/test_mix_rows_cpu.py holds the builder to that), alone and as row 5 of a tile whose input list has 11 entries,
    two chunks, with the row's terms in both"""
    x, m = ref.sensitive_case(512, seed=3)
    want = ref.mix_ref(x, m)
    ref.same_bits(run(x, m), want, 'sensitive row')
    assert np.all(ref.mix_ref(x[::-1], m[:, ::-1])[0] != want[0])
    assert np.all([ref.fused(x[:, i], m[0]) != want[0, i] for i in range(512)])
    wide = np.zeros((T, 11))
    wide[5, [1, 4, 9]] = m[0]                             # its terms in two chunks, other rows' terms between them
    wide[np.arange(T), np.arange(T)] += 0.5 * (np.arange(T) != 5) * (np.arange(T) != 1) * (np.arange(T) != 4)
    wide[0, 10], wide[6, 5], wide[6, 8] = 2.0, 0.25, -0.5
    assert ref.reads_of(wide, T) == 11
    xw = ref.rows_input(11, 512, 21, specials=False)
    xw[[1, 4, 9]] = x
    got = run(xw, wide)
    ref.same_bits(got, ref.mix_ref(xw, wide), 'sensitive row inside a tile')
    assert got[5].tobytes() == want[0].tobytes()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', [5, 1024, 4100, 4101])
def test_windows_and_guards(n, kind):
    """input and output rows as windows at an odd element offset of wider tensors with row stride n + 37 (odd for the
    even n: the rows of a tile alternate in alignment): the guards of both sides stay, the input is bit for bit what was
    put there"""
    dtype = NP_OF[kind]
    for name, m, off in (SHAPES[2], SHAPES[6], SHAPES[7], SHAPES[9]):       # iq-6, tridiagonal 2T+1, dense, long-row-17
        x = ref.rows_input(m.shape[1], n, 300 + n, dtype)
        src, dst = Window(m.shape[1], n, dtype, x), Window(m.shape[0], n, dtype)
        st = distortion.MixStage(m, n, offset=off, dtype=dtype)
        assert st.apply_torch(src.win, dst.win).data_ptr() == dst.ptr
        torch.cuda.synchronize()
        ref.same_bits(dst.host(), ref.mix_ref(x, m, off), f'window {name} n={n} {kind}')
        dst.assert_guards()
        src.assert_holds(x)
        st.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_stores_cover_the_row_and_nothing_else(kind):
    """an output full of a sentinel, the rows at every lead into a 16-byte slot: [0, n) of every row is overwritten
    (rows without terms too), nothing else is"""
    dtype, tdt = NP_OF[kind], torch.float64 if kind == 'f64' else torch.float32
    name, m, off = SHAPES[11]                            # empty-tile: 3 T rows, the middle tile without terms
    for n in (3, SPAN[kind] + 1):
        x = ref.rows_input(m.shape[1], n, 500 + n, dtype, specials=False)
        want = ref.mix_ref(x, m, off)
        assert not np.any(want == SENTINEL[kind])
        xd = torch.from_numpy(x).to(dev())
        st = distortion.MixStage(m, n, offset=off, dtype=dtype)
        for lead in range(16 // np.dtype(dtype).itemsize + 1):
            out = torch.full((m.shape[0], n + 40), SENTINEL[kind], dtype=tdt, device=dev())
            st.apply_torch(xd, out[:, lead:lead + n])
            full = out.cpu().numpy()
            ref.same_bits(full[:, lead:lead + n], want, f'{name} n={n} lead={lead} {kind}')
            assert np.all(full[:, :lead] == dtype(SENTINEL[kind])) and np.all(full[:, lead + n:] == dtype(SENTINEL[kind]))
        st.close()


@pytest.mark.parametrize('kind,side', [('f64', 'far_in'), ('f64', 'far_out'), ('f32', 'far_in')])
def test_rows_more_than_2_pow_32_elements_apart(kind, side):
    dtype, n = NP_OF[kind], 4099
    m, off = np.array([[1.02, -0.07], [0.05, 0.97]]), [0.01, -0.02]
    x = ref.rows_input(2, n, 900, dtype)
    want = ref.mix_ref(x, m, off)
    st = distortion.MixStage(m, n, offset=off, dtype=dtype)
    src = dst = None
    try:
        if side == 'far_in':
            src, dst = FarWindow(n, dtype, x), Window(2, n, dtype)
        else:
            src, dst = Window(2, n, dtype, x), FarWindow(n, dtype)
        assert max(src.stride, dst.stride) > 2**32
        assert st.apply_torch(src.win, dst.win).data_ptr() == dst.ptr
        torch.cuda.synchronize()
        ref.same_bits(dst.host(), want, f'far rows {kind} {side}')
        dst.assert_guards()
        src.assert_holds(x)
    finally:
        st.close()
        del src, dst
        free_far_arena()


def test_overlap_and_refused_tensors():
    n = 256
    st = distortion.MixStage(ref.dense(3, 5, 1), n)
    buf = torch.zeros(8 * n + 64, dtype=torch.float64, device=dev())
    x, out = buf[:5 * n].view(5, n), buf[5 * n:8 * n].view(3, n)
    st.apply_torch(x, out)                                                # side by side: fine
    for bad_out in (buf[:3 * n].view(3, n), buf[5 * n - 1:8 * n - 1].view(3, n), buf[4 * n:7 * n].view(3, n)):
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_torch(x, bad_out)
    assert _engine.lib().wfk_mix_rows_apply(st.plan._h, x.data_ptr(), n, x.data_ptr() + 8 * n, n, None) == -1
    assert b'mix rows is out of place: out overlaps in' in _engine.lib().wfk_last_error()
    for args, message in (((x.data_ptr(), n - 1, out.data_ptr(), n), b'stride smaller than n'),
                          ((x.data_ptr(), n, out.data_ptr(), n - 1), b'stride smaller than n'),
                          ((x.data_ptr() + 4, n, out.data_ptr(), n), b'not aligned to their element'),
                          ((None, n, out.data_ptr(), n), b'null in / out')):
        assert _engine.lib().wfk_mix_rows_apply(st.plan._h, *args, None) == -1
        assert message in _engine.lib().wfk_last_error(), (message, _engine.lib().wfk_last_error())
    xc = torch.zeros((5, n), dtype=torch.float64, device=dev())
    yc = torch.zeros((3, n), dtype=torch.float64, device=dev())
    for bad in (xc[:4], xc[:, :n - 1], xc.to(torch.float32), xc.cpu(), xc.t().contiguous().t()):
        with pytest.raises(ValueError):
            st.apply_torch(bad, yc)
    for bad in (yc[:2], yc[:, :n - 1], yc.to(torch.float32), yc.cpu(), yc.t().contiguous().t(), xc):
        with pytest.raises(ValueError):
            st.apply_torch(xc, bad)
    st.close()
    empty = distortion.MixStage(np.eye(2), 0)                             # n = 0: a no-op
    assert tuple(empty.apply_torch(torch.zeros((2, 0), dtype=torch.float64, device=dev())).shape) == (2, 0)
    assert _engine.lib().wfk_mix_rows_apply(empty.plan._h, None, 0, None, 0, None) == 0
    empty.close()


def test_consistency_of_the_entry_points():
    n = 3001
    for name, m, off in SHAPES:
        for kind in ('f64', 'f32'):
            st = distortion.MixStage(m, n, offset=off, dtype=NP_OF[kind])
            assert st.kernel_name() == f'mix_rows<{NAME_OF[kind]}>'
            assert st.reads == st.plan.library_reads() == ref.reads_of(m, T), name
            assert (st.rows_out, st.rows_in, st.nnz, st.n) == (m.shape[0], m.shape[1], np.count_nonzero(m), n)
            st.close()
    blocks, off = ref.iq_blocks(5, 30)
    x = ref.rows_input(10, n, 31)
    a = distortion.MixStage.from_blocks(blocks, n, offset=off)
    b = distortion.MixStage(ref.block_diagonal(blocks), n, offset=off)
    assert (a.reads, a.nnz, a.rows_out, a.rows_in) == (b.reads, b.nnz, 10, 10) and a.reads == 10
    xd = torch.from_numpy(x).to(dev())
    ya, yb = a.apply_torch(xd).cpu().numpy(), b.apply_torch(xd).cpu().numpy()
    want = ref.mix_ref(x, ref.block_diagonal(blocks), off)
    ref.same_bits(ya, want, 'from_blocks')
    ref.same_bits(yb, want, 'dense block-diagonal')
    for sig in (x, x.astype(np.float32)):
        ref.same_bits(distortion.mix_rows(sig, ref.block_diagonal(blocks), off), ref.mix_ref(sig, ref.block_diagonal(blocks), off),
                      f'mix_rows {sig.dtype}')
    xi = (ref.rows_input(10, 50, 35, specials=False) * 100).astype(np.int32)          # read as float64
    ref.same_bits(distortion.mix_rows(xi, ref.dense(4, 10, 32)), ref.mix_ref(xi.astype(np.float64), ref.dense(4, 10, 32)),
                  'integer input')
    for st in (a, b):
        st.close()
    if importlib.util.find_spec('scipy') is not None:
        import scipy.sparse as sp
        tri = ref.band(2 * T + 1, 1, 33)
        c = distortion.MixStage(sp.csr_matrix(tri), n)
        assert (c.nnz, c.reads) == (np.count_nonzero(tri), ref.reads_of(tri, T))
        xt = ref.rows_input(2 * T + 1, n, 34)
        ref.same_bits(c.apply_torch(torch.from_numpy(xt).to(dev())).cpu().numpy(), ref.mix_ref(xt, tri), 'scipy.sparse matrix')
        c.close()


def test_side_stream_equals_default_stream():
    name, m, off = SHAPES[7]
    n = 4099
    x = ref.rows_input(m.shape[1], n, 600)
    st = distortion.MixStage(m, n, offset=off)
    a = st.apply_torch(torch.from_numpy(x).to(dev())).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = st.apply_torch(torch.from_numpy(x).to(dev())) + 0             # produced and consumed on the side stream
    side.synchronize()
    want = ref.mix_ref(x, m, off)
    ref.same_bits(a, want, 'default stream')
    ref.same_bits(b.cpu().numpy(), want, 'side stream')
    st.close()


def test_pipeline_iq_correction_then_dac_codes():
    """the README's IQ pair, sampled on the device, through MixStage.from_blocks and DacStage(interleave=2): the codes
    are those of the referee chain mix_ref -> dac_ref on the sampled rows"""
    from waveforms_amd import cosPulse, gaussian
    from waveforms_amd._sampling import BatchSampler
    pulses = [200e-9, 900e-9, 1700e-9, 2600e-9]
    env = [sum((gaussian(40e-9) >> t0 for t0 in pulses[1:]), gaussian(40e-9) >> pulses[0]),
           sum((cosPulse(60e-9) >> t0 for t0 in pulses[1:]), cosPulse(60e-9) >> pulses[0])]
    gates = BatchSampler(env, ('linspace', 0.0, 4e-6, 8000, False)).launch_torch(
        torch.empty((2, 8000), dtype=torch.float64, device=dev()))
    block, leak = [[1.03, -0.045], [0.02, 0.96]], [0.004, -0.0025]
    mix = distortion.MixStage.from_blocks([block], 8000, offset=leak)
    dac = distortion.DacStage.from_full_scale(1.2, 8000, batch=2, bits=14, shift=2, interleave=2)
    counts = torch.empty((2, 3), dtype=torch.int64, device=dev())
    codes = dac.apply_torch(mix.apply_torch(gates), counts=counts).cpu().numpy()
    x = gates.cpu().numpy()
    want, want_counts = dac_rows_ref.dac_ref(ref.mix_ref(x, np.array(block), leak), dac.gain, dac.offset, 14, 2, 2)
    assert codes.shape == (1, 16000) and np.array_equal(codes, want) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert len(np.unique(codes)) > 100 and not want_counts.any()
    mix.close()
    dac.close()


def test_plain_c_consumer_mixes_on_the_device(tmp_path):
    exe = tmp_path / 'mix_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'mix_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'mixed on the device, 16 values ok' in r.stdout, r.stdout
