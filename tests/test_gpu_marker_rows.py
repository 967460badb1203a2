"""The marker stage on the device (distortion.MarkerStage / marker_rows, csrc/wfk_marker_rows.hip) against the referee
tests/marker_rows_ref.py, the NumPy statement of the semantics.  Markers, code bits and counts are integers: every
comparison here is exact, there is no tolerance.  Sizes follow the kernel's real geometry through `.span()`."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import marker_rows_ref as ref
from row_windows import FarWindow, Window, bits_equal, free_far_arena
from waveforms_amd import distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 'S-1', 'S', 'S+1', 10007]   # S: that form's span
EDGES = [(0, 0), (1, 0), (0, 1), (7, 63), (64, 65), (4096, 4095)]                            # (lead, trail) per row
NP_OF = {'f64': np.float64, 'f32': np.float32}
NAME_OF = {'f64': 'double', 'f32': 'float'}
FORMS = ('bytes', 'codes')
SENTINEL = -21846                                                                            # 0xAAAA, 0xAA as a byte


def dev():
    return torch.device('cuda', torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def span(form, k):
    st = distortion.MarkerStage(8, batch=k, group=k)
    try:
        return st.span(codes=form == 'codes')
    finally:
        st.close()


def random_codes(rows, n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (rows, n)).astype(np.int16)


def run(x, lead, trail, threshold=0.0, k=1, form='bytes', counts=True, bit=0, codes=None):
    """x (rows, n) NumPy -> (markers uint8, or the codes with `bit` written; counts or None) of a stage built for it,
    counts from a tensor full of garbage"""
    n = x.shape[1]
    st = distortion.MarkerStage(n, lead, trail, threshold, group=k, dtype=x.dtype, batch=x.shape[0])
    try:
        c = torch.full((st.out_rows, 2), 0x5a5a5a5a5a, dtype=torch.int64, device=dev()) if counts else None
        xd = torch.from_numpy(x).to(dev())
        if form == 'codes':
            cd = torch.from_numpy(codes).to(dev())
            y = st.apply_codes_torch(xd, cd, bit=bit, counts=c)
            assert y.dtype == torch.int16 and tuple(y.shape) == (st.out_rows, k * n) and y.data_ptr() == cd.data_ptr()
        else:
            y = st.apply_torch(xd, counts=c)
            assert y.dtype == torch.uint8 and tuple(y.shape) == (st.out_rows, n)
        return y.cpu().numpy(), (c.cpu().numpy() if counts else None)
    finally:
        st.close()


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}; last at {tuple(bad[-1])}')


def check(x, lead, trail, threshold, k, form, what, bit=0, seed=1):
    """one apply with counts against the referee -> (markers of the referee, its counts)"""
    want_m, want_counts = ref.marker_ref(x, lead, trail, threshold, k)
    if form == 'codes':
        codes = random_codes(x.shape[0] // k, k * x.shape[1], seed)
        got, counts = run(x, lead, trail, threshold, k, form, bit=bit, codes=codes)
        same(got, ref.into_codes(codes, want_m, k, bit), what)
    else:
        got, counts = run(x, lead, trail, threshold, k, form)
        same(got, want_m, what)
    same(counts, want_counts, what + ', counts')
    return want_m, want_counts


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('size', SIZES)
def test_small_shapes(size, kind):
    rows, dtype = 6, NP_OF[kind]
    for form in FORMS:
        for k in (1, 2):
            S = span(form, k)
            assert S == {('bytes', 1): 16384, ('bytes', 2): 16384, ('codes', 1): 8192, ('codes', 2): 4096}[form, k]
            n = size if isinstance(size, int) else S + {'S-1': -1, 'S': 0, 'S+1': 1}[size]
            st = distortion.MarkerStage(n, [e[0] for e in EDGES[:rows // k]], [e[1] for e in EDGES[:rows // k]], 0.25,
                                        group=k, dtype=dtype)
            for codes in (False, True):
                for counts in (False, True):
                    assert st.kernel_name(codes=codes, counts=counts) == (
                        f'marker_rows{"_codes" if codes else ""}{"_count" if counts else ""}<{NAME_OF[kind]}>')
            assert (st.n, st.batch, st.group, st.out_rows, st.dtype) == (n, rows, k, rows // k, np.dtype(dtype))
            assert st.lead.tolist() == [e[0] for e in EDGES[:rows // k]] and st.threshold.tolist() == [0.25] * (rows // k)
            assert st.trail.tolist() == [e[1] for e in EDGES[:rows // k]]
            st.close()
            for half in range(k):                                  # k = 2 has 3 marker rows: the six edges in two runs
                edges = EDGES[half * rows // k:(half + 1) * rows // k]
                lead, trail = [e[0] for e in edges], [e[1] for e in edges]
                for pattern, threshold in (('bursts', 0.0), ('bursts', 0.25), ('specials', 0.25), ('specials', 0.0)):
                    x = ref.rows_pattern(rows, n, 100 + n + half, pattern, dtype, threshold, burst=9, gap=60)
                    what = f'n={n} {kind} {form} k={k} {pattern} threshold={threshold} edges={edges}'
                    want_m, _ = check(x, lead, trail, threshold, k, form, what, bit=(n + half) % 16, seed=n)
                    if n >= 255 and pattern == 'bursts' and half == 0:   # markers, and gaps between them ((0, 0) is there)
                        assert want_m.any() and not want_m.all(), what


@pytest.mark.parametrize('form,k,kind', [('bytes', 1, 'f64'), ('codes', 1, 'f32'), ('codes', 2, 'f64'), ('bytes', 2, 'f32')])
def test_workgroup_edges(form, k, kind):
    """single spikes one sample before, at and after a workgroup boundary: the mark appears in the neighbouring workgroup
    exactly `lead` before and `trail` after the spike -- at S = 4096 (codes, k = 2) a 4096 edge crosses a whole
    neighbour's span and ends in the one beyond"""
    S = span(form, k)
    n = 3 * S + 11
    at = [s * S + d for s in (1, 2) for d in (-1, 0, 1)]
    rows = len(at) * k
    x = ref.rows_pattern(rows, n, 0, 'spikes', NP_OF[kind], positions=[[p] if r % k == k - 1 else [] for p in at
                                                                         for r in range(k)])
    assert np.count_nonzero(x) == len(at)
    for lead, trail in ((0, 0), (5, 0), (0, 5), (63, 64), (4096, 0), (0, 4096), (4096, 4096)):
        what = f'edges {form} k={k} {kind} lead={lead} trail={trail}'
        want_m, want_counts = check(x, lead, trail, 0.0, k, form, what, bit=3)
        if form == 'codes':                                        # by index too, from the form under test
            codes = random_codes(rows // k, k * n, 5)
            got = ((run(x, lead, trail, 0.0, k, form, bit=3, codes=codes)[0][:, ::k] >> 3) & 1).astype(np.uint8)
        else:
            got, _ = run(x, lead, trail, 0.0, k, form)
        for g, p in enumerate(at):
            lo, hi = max(p - lead, 0), p + trail                   # (a 4096 lead from S - 1 = 4095 is cut at the row's start)
            assert hi + 2 < n
            for q in (lo - 2, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, hi + 2):
                if q >= 0:
                    assert got[g, q] == (lo <= q <= hi), (what, g, p, q)
            assert int(got[g].sum()) == hi - lo + 1, (what, g)
        assert want_counts[:, 1].tolist() == [1] * len(at)


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('n', [5, 256, 4099])
def test_windows_and_canaries(n, k, kind):
    """input rows 8 and 40 bytes into a wider buffer with stride n + 37; every output lead 0 .. 15 bytes and 0 .. 7
    codes, output stride row + 64: sentinels before, after and between the output rows stay, the input is intact bit
    for bit, codes pre-filled with random int16 keep every bit but `bit`, a counts tensor full of garbage comes out
    exact, and a second apply neither changes the codes nor adds to the counts"""
    dtype = NP_OF[kind]
    tdt = torch.float64 if kind == 'f64' else torch.float32
    rows, bit = 6, 5
    x = ref.rows_pattern(rows, n, 400 + n, 'bursts', dtype, 0.25, burst=7, gap=30)
    edges = (EDGES[1:] + EDGES[:1])[:rows // k]
    lead, trail = [e[0] for e in edges], [e[1] for e in edges]
    st = distortion.MarkerStage(n, lead, trail, 0.25, group=k, dtype=dtype)
    want, want_counts = ref.marker_ref(x, lead, trail, 0.25, k)
    assert n < 256 or (want.any() and want_counts[:, 1].min() >= 1)
    raw = np.uint64 if kind == 'f64' else np.uint32
    for off_bytes in (8, 40):
        off = off_bytes // np.dtype(dtype).itemsize
        wide = torch.full((rows, n + 37), 7.0, dtype=tdt, device=dev())
        win = wide[:, off:off + n]
        win.copy_(torch.from_numpy(x))
        before = wide.cpu().numpy().view(raw).copy()
        for shift in range(16):                                                     # bytes
            out = torch.full((rows // k, n + 64), 0xAA, dtype=torch.uint8, device=dev())
            counts = torch.full((rows // k, 2), -77, dtype=torch.int64, device=dev())
            res = st.apply_torch(win, out[:, shift:shift + n], counts)
            assert res.data_ptr() == out[:, shift:].data_ptr() and tuple(res.shape) == (rows // k, n)
            full = out.cpu().numpy()
            same(full[:, shift:shift + n], want, f'bytes window n={n} k={k} {kind} lead={shift} off={off_bytes}')
            assert np.all(full[:, :shift] == 0xAA) and np.all(full[:, shift + n:] == 0xAA)
            same(counts.cpu().numpy(), want_counts, f'counts n={n} k={k} {kind} lead={shift}')
        for shift in range(8):                                                      # codes
            filled = random_codes(rows // k, k * n, 17 * shift + n)
            out = torch.full((rows // k, k * n + 64), SENTINEL, dtype=torch.int16, device=dev())
            out[:, shift:shift + k * n] = torch.from_numpy(filled).to(dev())
            counts = torch.full((rows // k, 2), -77, dtype=torch.int64, device=dev())
            res = st.apply_codes_torch(win, out[:, shift:shift + k * n], bit, counts)
            assert res.data_ptr() == out[:, shift:].data_ptr() and tuple(res.shape) == (rows // k, k * n)
            full = out.cpu().numpy()
            got = full[:, shift:shift + k * n]
            assert not np.any((got.view(np.uint16) ^ filled.view(np.uint16)) & ~np.uint16(1 << bit))
            same(got, ref.into_codes(filled, want, k, bit), f'codes window n={n} k={k} {kind} lead={shift} off={off_bytes}')
            assert np.all(full[:, :shift] == SENTINEL) and np.all(full[:, shift + k * n:] == SENTINEL)
            same(counts.cpu().numpy(), want_counts, f'codes counts n={n} k={k} {kind} lead={shift}')
            st.apply_codes_torch(win, out[:, shift:shift + k * n], bit, counts)      # overwrites, does not accumulate
            assert np.array_equal(out.cpu().numpy(), full)
            same(counts.cpu().numpy(), want_counts, f'counts of a second apply n={n} k={k} {kind} lead={shift}')
        assert np.array_equal(wide.cpu().numpy().view(raw), before)
    st.close()


def test_far_rows():
    """float64 input rows, then int16 code rows, more than 2^32 elements apart (the other side an ordinary window):
    results and counts as the referee has them, every guard untouched, the input bit for bit what was put there"""
    n, edge, bit = 2**17 - 3, 100, 1
    x = ref.rows_pattern(2, n, 900, 'bursts', np.float64, burst=50, gap=5000)
    codes = random_codes(2, n, 901)
    want_m, want_counts = ref.marker_ref(x, edge, edge)
    want = ref.into_codes(codes, want_m, 1, bit)
    assert want_counts[:, 1].min() > 5
    st = distortion.MarkerStage(n, edge, edge, batch=2)
    try:
        for far_side in ('x', 'codes'):
            src = FarWindow(n, np.float64, x) if far_side == 'x' else Window(2, n, np.float64, x)
            dst = FarWindow(n, np.int16, codes) if far_side == 'codes' else Window(2, n, np.int16, codes)
            counts = torch.full((2, 2), -77, dtype=torch.int64, device=dev())
            assert st.apply_codes_torch(src.win, dst.win, bit, counts).data_ptr() == dst.ptr
            same(dst.host(), want, f'far {far_side}')
            same(counts.cpu().numpy(), want_counts, f'far {far_side}, counts')
            dst.assert_guards()
            src.assert_holds(x)
            if far_side == 'x':                                      # and the bytes form from the far rows
                out = Window(2, n, np.int16)                         # (a window of int16 read as bytes: 2 n of them a row)
                y = out.win.view(torch.uint8)[:, :n]
                st.apply_torch(src.win, y, counts)
                same(y.cpu().numpy(), want_m, 'far x, bytes')
                same(counts.cpu().numpy(), want_counts, 'far x, bytes, counts')
                assert bits_equal(out.host()[:, (n + 1) // 2:], np.full((2, n - (n + 1) // 2), out.sentinel, dtype=np.int16))
                out.assert_guards()
                src.assert_holds(x)
            del src, dst
    finally:
        st.close()
        free_far_arena()


@pytest.mark.parametrize('kind,k', [('f64', 1), ('f32', 2)])
def test_many_workgroups_per_row(kind, k):
    """64 x 100003, sparse bursts: markers and counts exact per marker row in both forms, the rows' counts all different"""
    rows, n = 64, 100003
    x = ref.rows_pattern(rows, n, 700, 'bursts', NP_OF[kind], burst=30, gap=4000)
    lead = [(7 * g) % 90 for g in range(rows // k)]
    trail = [(11 * g) % 70 for g in range(rows // k)]
    for form in FORMS:
        _, want_counts = check(x, lead, trail, 0.0, k, form, f'{rows} x {n} {kind} k={k} {form}', bit=0)
    assert want_counts[:, 1].min() >= 10
    assert len({tuple(c) for c in want_counts.tolist()}) == rows // k


@pytest.mark.parametrize('n', [257, 10007])
def test_row_independence(n):
    """a row's markers and counts are the same alone, first and last in a batch; with k = 2 a pair is the OR of the two
    single-row results at lead = trail = 0"""
    x = ref.rows_pattern(1, n, 500 + n, 'bursts', burst=9, gap=80)
    others = ref.rows_pattern(4, n, 501 + n, 'bursts', burst=20, gap=50)
    alone, c_alone = run(x, [9], [4])
    want, want_counts = ref.marker_ref(x, 9, 4)
    same(alone, want, 'alone')
    same(c_alone, want_counts, 'alone, counts')
    first, c_first = run(np.vstack([x, others]), [9, 0, 100, 3, 64], [4, 1, 0, 200, 64])
    last, c_last = run(np.vstack([others, x]), [0, 100, 3, 64, 9], [1, 0, 200, 64, 4])
    assert np.array_equal(first[0], alone[0]) and np.array_equal(c_first[0], c_alone[0])
    assert np.array_equal(last[4], alone[0]) and np.array_equal(c_last[4], c_alone[0])
    a, _ = run(x, 0, 0)
    b, _ = run(others[:1], 0, 0)
    for pair in (np.vstack([x, others[:1]]), np.vstack([others[:1], x])):
        both, c_both = run(pair, 0, 0, k=2)
        assert np.array_equal(both, a | b) and np.array_equal(c_both, ref.counts_of(a | b))
    assert np.any(a != b)


def test_side_stream_equals_default_stream():
    n, rows, k = 4099, 6, 2
    x = ref.rows_pattern(rows, n, 600, 'bursts', burst=9, gap=100)
    codes = random_codes(rows // k, k * n, 601)
    st = distortion.MarkerStage(n, 20, 10, group=k, batch=rows)
    xd, cd = torch.from_numpy(x).to(dev()), torch.from_numpy(codes).to(dev())
    ca = torch.empty((rows // k, 2), dtype=torch.int64, device=dev())
    a = st.apply_codes_torch(xd, cd, 0, ca).cpu().numpy()
    ma = st.apply_torch(xd).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z, zc = torch.from_numpy(x).to(dev()), torch.from_numpy(codes).to(dev())
        cb = torch.full((rows // k, 2), 99, dtype=torch.int64, device=dev())
        b = st.apply_codes_torch(z, zc, 0, cb) + 0                  # produced and consumed on the side stream
        mb = st.apply_torch(z) + 0
        cb = cb + 0
    side.synchronize()
    want_m, want_counts = ref.marker_ref(x, 20, 10, 0.0, k)
    want = ref.into_codes(codes, want_m, k, 0)
    same(a, want, 'default stream')
    same(b.cpu().numpy(), want, 'side stream')
    same(ma, want_m, 'default stream, bytes')
    same(mb.cpu().numpy(), want_m, 'side stream, bytes')
    same(ca.cpu().numpy(), want_counts, 'default stream, counts')
    same(cb.cpu().numpy(), want_counts, 'side stream, counts')
    st.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_counts_absent(kind):
    n, rows = 8193, 4
    x = ref.rows_pattern(rows, n, 650, 'bursts', NP_OF[kind], burst=9, gap=100)
    for k in (1, 2):
        st = distortion.MarkerStage(n, 33, 12, group=k, dtype=NP_OF[kind], batch=rows)
        assert st.kernel_name() == st.kernel_name(codes=False, counts=False) == f'marker_rows<{NAME_OF[kind]}>'
        assert st.kernel_name(codes=True) == f'marker_rows_codes<{NAME_OF[kind]}>'
        st.close()
        want_m, want_counts = ref.marker_ref(x, 33, 12, 0.0, k)
        codes = random_codes(rows // k, k * n, 651)
        for form, want in (('bytes', want_m), ('codes', ref.into_codes(codes, want_m, k, 9))):
            plain, none = run(x, 33, 12, 0.0, k, form, counts=False, bit=9, codes=codes)
            counted, counts = run(x, 33, 12, 0.0, k, form, bit=9, codes=codes)
            assert none is None
            same(plain, want, f'without counts {kind} k={k} {form}')
            same(counted, want, f'with counts {kind} k={k} {form}')
            same(counts, want_counts, f'counts {kind} k={k} {form}')


def test_overlap_and_refused_tensors():
    n, rows = 256, 4
    st = distortion.MarkerStage(n, 3, 2, group=2, batch=rows)
    buf = torch.zeros(rows * n + 64, dtype=torch.float64, device=dev())
    x = buf[:rows * n].view(rows, n)
    as_bytes, as_codes = buf.view(torch.uint8), buf.view(torch.int16)          # the same bytes
    out = torch.zeros((2, n), dtype=torch.uint8, device=dev())
    codes = torch.zeros((2, 2 * n), dtype=torch.int16, device=dev())
    counts = torch.zeros((2, 2), dtype=torch.int64, device=dev())
    st.apply_torch(x, out, counts)                                             # fine
    st.apply_codes_torch(x, codes, 0, counts)
    for bad_out in (as_bytes[:2 * n].view(2, n), as_bytes[8 * rows * n - 2 * n + 8:][:2 * n].view(2, n)):
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_torch(x, bad_out, counts)
    for bad_codes in (as_codes[:4 * n].view(2, 2 * n), as_codes[4 * rows * n - 4 * n + 8:][:4 * n].view(2, 2 * n)):
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_codes_torch(x, bad_codes, 0, counts)
    over_x = buf[8:12].view(torch.int64).view(2, 2)
    over_out = out.view(-1)[16:48].view(torch.int64).view(2, 2)
    over_codes = codes.view(-1)[16:32].view(torch.int64).view(2, 2)
    for bad_counts in (over_x, over_out):
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_torch(x, out, bad_counts)
    for bad_counts in (over_x, over_codes):
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_codes_torch(x, codes, 0, bad_counts)
    wide = torch.zeros((2, 3), dtype=torch.int64, device=dev())
    for bad_counts in (counts[:1], counts.view(-1), wide[:, :2], counts.to(torch.int32), counts.to(torch.float64),
                       counts.cpu(), torch.zeros((2, 3), dtype=torch.int64, device=dev())):
        with pytest.raises(ValueError, match='counts'):
            st.apply_torch(x, out, bad_counts)
        with pytest.raises(ValueError, match='counts'):
            st.apply_codes_torch(x, codes, 0, bad_counts)
    xc = torch.zeros((rows, n), dtype=torch.float64, device=dev())
    for bad in (xc[:2], xc[:, :n - 1], xc.to(torch.float32), xc.cpu(), xc.t().contiguous().t()):
        with pytest.raises(ValueError):
            st.apply_torch(bad, out)
        with pytest.raises(ValueError):
            st.apply_torch(bad)
        with pytest.raises(ValueError):
            st.apply_codes_torch(bad, codes)
    for bad in (out[:1], out[:, :n - 1], out.to(torch.int16), out.cpu(), out.t().contiguous().t(),
                torch.zeros((rows, n), dtype=torch.uint8, device=dev())):
        with pytest.raises(ValueError):
            st.apply_torch(xc, bad)
    for bad in (codes[:1], codes[:, :2 * n - 1], codes.to(torch.int32), codes.cpu(), codes.t().contiguous().t(),
                torch.zeros((rows, n), dtype=torch.int16, device=dev())):
        with pytest.raises(ValueError):
            st.apply_codes_torch(xc, bad)
    for bit in (-1, 16):
        with pytest.raises(ValueError, match='bit'):
            st.apply_codes_torch(xc, codes, bit)
    st.close()
    empty = distortion.MarkerStage(0, 5, 5, group=2, batch=2)                   # n = 0: a no-op that zeroes the counts
    e = torch.zeros((2, 0), dtype=torch.float64, device=dev())
    c = torch.full((1, 2), 5, dtype=torch.int64, device=dev())
    assert tuple(empty.apply_torch(e, counts=c).shape) == (1, 0)
    assert not c.cpu().numpy().any()
    c.fill_(7)
    assert tuple(empty.apply_codes_torch(e, torch.zeros((1, 0), dtype=torch.int16, device=dev()), 3, c).shape) == (1, 0)
    assert not c.cpu().numpy().any()
    empty.close()


def test_library_refuses_a_bad_apply():
    """the C side's own checks of an apply, through the raw pointers: a bit outside 0 .. 15, a stride below the row,
    rows not aligned to their element, overlap; nothing is launched"""
    from waveforms_amd import _engine
    n = 64
    st = distortion.MarkerStage(n, 1, 1, batch=2)
    x = torch.zeros((2, n), dtype=torch.float64, device=dev())
    codes = torch.zeros((2, n), dtype=torch.int16, device=dev())
    out = torch.zeros((2, n), dtype=torch.uint8, device=dev())
    counts = torch.zeros((2, 2), dtype=torch.int64, device=dev())
    lib = _engine.lib()
    h = st.plan._h
    for bit in (-1, 16):
        assert lib.wfk_marker_rows_apply_codes(h, x.data_ptr(), n, codes.data_ptr(), n, bit, None, None) == -1
        assert b'bit must lie in [0, 15]' in lib.wfk_last_error()
    for args, message in (((x.data_ptr(), n - 1, out.data_ptr(), n, None), 'stride smaller'),
                          ((x.data_ptr(), n, out.data_ptr(), n - 1, None), 'stride smaller'),
                          ((x.data_ptr() + 4, n, out.data_ptr(), n, None), 'not aligned'),
                          ((x.data_ptr(), n, x.data_ptr() + 8, n, None), 'overlaps'),
                          ((x.data_ptr(), n, out.data_ptr(), n, out.data_ptr() + 8), 'overlaps'),
                          ((x.data_ptr(), n, out.data_ptr(), n, x.data_ptr() + 16), 'overlaps'),
                          ((x.data_ptr(), n, out.data_ptr(), n, counts.data_ptr() + 4), 'not aligned'),
                          ((None, n, out.data_ptr(), n, None), 'null')):
        with pytest.raises(_engine.EngineError, match=message):
            st.apply(*args)
    for args, message in (((x.data_ptr(), n, codes.data_ptr() + 1, n, 0), 'not aligned'),
                          ((x.data_ptr(), n, codes.data_ptr(), n - 1, 0), 'stride smaller'),
                          ((x.data_ptr(), n, x.data_ptr() + 2, n, 0), 'overlaps')):
        with pytest.raises(_engine.EngineError, match=message):
            st.apply_codes(*args)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any() and not codes.cpu().numpy().any()
    st.close()
    empty = distortion.MarkerStage(0, 1, 1, batch=2)                               # n = 0: null rows, the report zeroed
    for call in (lambda c: lib.wfk_marker_rows_apply(empty.plan._h, None, 0, None, 0, c, None),
                 lambda c: lib.wfk_marker_rows_apply_codes(empty.plan._h, None, 0, None, 0, 3, c, None)):
        counts.fill_(7)
        assert call(counts.data_ptr()) == 0 and call(None) == 0
        torch.cuda.synchronize()
        assert not counts.cpu().numpy().any()
        assert call(counts.data_ptr() + 4) == -1 and b'counts are not aligned' in lib.wfk_last_error()
    empty.close()


def test_numpy_round_trip():
    rows, n = 6, 3001
    x = ref.rows_pattern(rows, n, 800, 'bursts', burst=9, gap=100)
    for k in (1, 2):
        lead, trail = list(range(3, 3 + rows // k)), [2] * (rows // k)
        want_m, want_counts = ref.marker_ref(x, lead, trail, 0.0, k)
        same(distortion.marker_rows(x, lead, trail, group=k), want_m, f'marker_rows k={k}')
        m, counts = distortion.marker_rows(x, lead, trail, group=k, return_counts=True)
        same(m, want_m, f'marker_rows with counts k={k}')
        same(counts, want_counts, f'marker_rows counts k={k}')
        codes = random_codes(rows // k, k * n, 801)
        keep = codes.copy()
        got, counts = distortion.marker_rows(x, lead, trail, group=k, codes=codes, bit=2, return_counts=True)
        same(got, ref.into_codes(codes, want_m, k, 2), f'marker_rows into codes k={k}')
        same(counts, want_counts, f'marker_rows into codes, counts k={k}')
        assert np.array_equal(codes, keep)                                          # a copy: the argument is not written
    x32 = ref.rows_pattern(rows, n, 802, 'bursts', np.float32, 0.1, burst=9, gap=100)
    same(distortion.marker_rows(x32, 20, 10, threshold=0.1), ref.marker_ref(x32, 20, 10, 0.1)[0], 'float32 rows, scalars')
    xi = (ref.rows_pattern(rows, 50, 803, 'bursts', burst=3, gap=9) * 100).astype(np.int32)
    same(distortion.marker_rows(xi, 1, 1), ref.marker_ref(xi.astype(np.float64), 1, 1)[0], 'integer input')


def test_end_to_end_gates_into_dac_codes():
    """the README example: pairs I, Q of gaussian / cosPulse pulses sampled on a 2 GS/s grid (exact zeros outside the
    pulses), quantised to 14 bits left-justified, the switch marker of each pair written into bit 0"""
    from waveforms_amd import cosPulse, gaussian
    from waveforms_amd._sampling import BatchSampler
    n, rate, pairs, lead, trail = 8000, 2e9, 3, 20, 10
    starts = [200e-9, 900e-9, 1700e-9, 2600e-9, 3400e-9][:4]                        # spacing far above lead + trail
    chans = []
    for p in range(pairs):
        i_row = sum(((gaussian(40e-9 + 10e-9 * p) >> t0) for t0 in starts[1:]), gaussian(40e-9) >> starts[0]) * 0.8
        q_row = sum(((cosPulse(60e-9) >> (t0 + 5e-9)) for t0 in starts[1:]), cosPulse(60e-9) >> (starts[0] + 5e-9)) * 0.5
        chans += [i_row, q_row]
    gates = BatchSampler(chans, ('linspace', 0.0, n / rate, n, False)).launch_torch(
        torch.empty((2 * pairs, n), dtype=torch.float64, device=dev()))
    dac = distortion.DacStage.from_full_scale(1.0, n, batch=2 * pairs, bits=14, shift=2, interleave=2)
    codes = dac.apply_torch(gates)
    before = codes.cpu().numpy().copy()
    assert not np.any(before & 3)
    mk = distortion.MarkerStage(n, lead=lead, trail=trail, group=2, batch=2 * pairs)
    counts = torch.empty((pairs, 2), dtype=torch.int64, device=dev())
    res = mk.apply_codes_torch(gates, codes, bit=0, counts=counts)
    assert res.data_ptr() == codes.data_ptr()
    after = codes.cpu().numpy()
    g = gates.cpu().numpy()
    want_m, want_counts = ref.marker_ref(g, lead, trail, 0.0, 2)
    assert np.array_equal(after >> 2, before >> 2) and not np.any(after & 2)
    assert np.array_equal(after & 1, np.repeat(want_m, 2, axis=1).astype(np.int16))
    same(counts.cpu().numpy(), want_counts, 'end to end, counts')
    assert want_counts[:, 1].tolist() == [len(starts)] * pairs
    assert np.count_nonzero(g == 0.0) > g.size // 2                                 # exact zeros between the pulses
    dac.close()
    mk.close()


def test_plain_c_consumer_marks_on_the_device(tmp_path):
    exe = tmp_path / 'marker_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'marker_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'marked on the device, parity ok' in r.stdout, r.stdout
