"""The curve stage on the device (distortion.CurveStage / interp_rows, csrc/wfk_curve_rows.hip) against the referee
tests/curve_rows_ref.py, the NumPy statement of np.interp's arithmetic.  The formula rounds a difference, a product and a
sum without fusing them, the search is exact and the counts are integers: every comparison here is of bits, there is no
tolerance."""
import contextlib
import os
import subprocess

import numpy as np
import pytest
import torch

import curve_rows_ref as ref
import dac_rows_ref
from cases import FP64_IIR_TOL
from graph_replay import eager, replay, sentinels_left
from row_windows import FarWindow, Window, bits_equal, free_far_arena
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_OF = {'f64': np.float64, 'f32': np.float32}
NAME_OF = {'f64': 'double', 'f32': 'float'}
SPAN = {'f64': 2048, 'f32': 4096}                       # samples one workgroup's span covers
KS = [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024]


@pytest.fixture(scope='module', autouse=True)
def far_arena():
    """the far rows' arena goes back to the device when the module is done"""
    yield
    free_far_arena()


def sizes(kind):
    S = SPAN[kind]
    return [1, 2, 3, 7, 8, 9, 1023, 1024, 1025, S - 1, S, S + 1, 10007]


def dev():
    return torch.device('cuda', torch.cuda.current_device())


@contextlib.contextmanager
def switches(**env):
    """the plan's experiment switches (WFK_CURVE_SPANS, WFK_CURVE_BUCKETS), read when a plan is made"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def all_curves():
    """every K of KS, uniform and log-spaced: 20 rows of one ragged batch"""
    pairs = [ref.knots(K, spacing) for K in KS for spacing in ('uniform', 'log')]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def run(x, xs, fs, left=None, right=None, counts=True, in_place=False):
    """x (rows, n) NumPy -> (y, counts or None, the stage's kernel name) of a stage built for it; counts from a tensor
    full of garbage"""
    st = distortion.CurveStage(xs, fs, x.shape[1], batch=x.shape[0], left=left, right=right, dtype=x.dtype)
    try:
        assert (st.batch, st.n) == x.shape
        c = torch.full((x.shape[0], 3), 0x5a5a5a5a5a, dtype=torch.int64, device=dev()) if counts else None
        xd = torch.from_numpy(x).to(dev())
        y = st.apply_torch(xd, out=xd if in_place else None, counts=c)
        assert (y.data_ptr() == xd.data_ptr()) == in_place and tuple(y.shape) == x.shape
        got = y.cpu().numpy()
        if not in_place:
            assert bits_equal(xd.cpu().numpy(), x), 'an out-of-place apply wrote its input'
        return got, (c.cpu().numpy() if counts else None), st.kernel_name(counts)
    finally:
        st.close()


def same_counts(got, want, what):
    assert got.dtype == want.dtype == np.int64 and np.array_equal(got, want), (what, got.tolist(), want.tolist())


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_small_shapes(kind):
    """every n around the slot, the wave and the span, every K around the bucket sizes, both spacings, as one ragged
    batch of 20 rows per n; for two of the sizes every curve again as a plan of its own, whose LDS is sized to it"""
    xs, fs = all_curves()
    for n in sizes(kind):
        x = ref.rows_input(n, xs, 100 + n, NP_OF[kind])
        got, counts, name = run(x, xs, fs)
        assert name == f'curve_rows_counts<{NAME_OF[kind]}>'
        ref.same_bits(got, ref.curve_ref(x, xs, fs), f'n={n} {kind}')
        same_counts(counts, ref.counts_ref(x, xs), f'counts n={n} {kind}')
        if n in (1025, 10007):
            for r, (xp, fp) in enumerate(zip(xs, fs)):
                one, c1, _ = run(x[r:r + 1], [xp], [fp])
                ref.same_bits(one, ref.curve_ref(x[r:r + 1], [xp], [fp]), f'alone n={n} {kind} K={len(xp)} row {r}')
                assert bits_equal(one[0], got[r]) and np.array_equal(c1[0], counts[r])
    st = distortion.CurveStage(xs, fs, 64, dtype=NP_OF[kind])
    assert st.knots.tolist() == [K for K in KS for _ in range(2)] and (st.batch, st.n) == (20, 64)
    st.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_ragged_batch_and_one_shared_curve(kind):
    xs, fs = ref.ragged_batch()
    for n in (9, SPAN[kind] + 1, 10007):
        x = ref.rows_input(n, xs, 200 + n, NP_OF[kind])
        got, counts, _ = run(x, xs, fs)
        ref.same_bits(got, ref.curve_ref(x, xs, fs), f'ragged n={n} {kind}')
        same_counts(counts, ref.counts_ref(x, xs), f'ragged counts n={n} {kind}')
    xp, fp = ref.uniform_knots(65)                       # k / 32: the knots are float32 values too, and samples hit them
    x = ref.rows_input(5000, [xp] * 4, 300, NP_OF[kind])
    assert np.count_nonzero(np.isin(x.astype(np.float64), xp)) > 100
    got, counts, _ = run(x, xp, fp)                      # one 1-D pair for every row
    ref.same_bits(got, ref.curve_ref(x, xp, fp), f'shared curve {kind}')
    same_counts(counts, ref.counts_ref(x, xp), f'shared curve counts {kind}')


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_special_values_ends_and_counts(kind):
    """NaN, +-inf, samples beyond both ends and +-0.0, with explicit ends -- left = right = NaN among them -- and the
    counts: exact, absent without a tensor, overwritten by a second apply"""
    xs, fs = ref.ragged_batch()
    xs, fs = xs + [np.array([0.0, 1.0])], fs + [np.array([-0.0, 5.0])]          # -0.0 at a knot that is 0.0
    n = 3 * SPAN[kind] + 5
    x = ref.rows_input(n, xs, 400, NP_OF[kind])
    x[:, :6] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300 if kind == 'f64' else 1e30])
    want_counts = ref.counts_ref(x, xs)
    assert want_counts.min() >= 1
    for left, right in ((None, None), (np.nan, np.nan), ([1.5, -np.inf, np.nan, 7.0], [np.inf, 2.5, -0.0, np.nan])):
        want = ref.curve_ref(x, xs, fs, left, right)
        got, counts, name = run(x, xs, fs, left, right)
        assert name == f'curve_rows_counts<{NAME_OF[kind]}>'
        ref.same_bits(got, want, f'special values {kind} ends={left}')
        same_counts(counts, want_counts, f'counts {kind} ends={left}')
        plain, none, name = run(x, xs, fs, left, right, counts=False)
        assert none is None and name == f'curve_rows<{NAME_OF[kind]}>'
        ref.same_bits(plain, want, f'without counts {kind} ends={left}')
    assert np.signbit(got[3, 3:5]).all() and not got[3, 3:5].any()              # fp[0] = -0.0 comes out as -0.0
    st = distortion.CurveStage(xs, fs, n, dtype=NP_OF[kind])
    xd, c = torch.from_numpy(x).to(dev()), torch.full((4, 3), -77, dtype=torch.int64, device=dev())
    y = st.apply_torch(xd, counts=c)
    same_counts(c.cpu().numpy(), want_counts, 'first apply')
    st.apply_torch(xd, out=y, counts=c)                                         # overwrites, does not accumulate
    same_counts(c.cpu().numpy(), want_counts, 'second apply')
    st.apply_torch(y, counts=c)                                                 # other data: other counts
    same_counts(c.cpu().numpy(), ref.counts_ref(y.cpu().numpy(), xs), 'third apply, on the output')
    st.close()


@pytest.mark.parametrize('spacing', ['log', 'uniform'])
def test_every_knot_and_its_neighbours(spacing):
    """K = 1024: every knot, the double below it and the double above it are inputs -- the search and its fix-up are exact;
    the same with the bucket table switched off (plain bisection) and with workgroups that walk three spans"""
    xp, fp = ref.knots(1024, spacing)
    edges = ref.knot_edges(xp)
    x = np.stack([edges, edges[::-1], np.random.default_rng(1).permutation(edges)])
    want = ref.curve_ref(x, xp, fp, -9.0, 9.0)
    assert np.count_nonzero(want == -9.0) == 3 and np.count_nonzero(want == 9.0) == 3      # one step off either end
    for env in ({}, {'WFK_CURVE_BUCKETS': 0}, {'WFK_CURVE_SPANS': 3}):
        with switches(**env):
            got, counts, _ = run(x, xp, fp, -9.0, 9.0)
        ref.same_bits(got, want, f'knot edges {spacing} {env}')
        same_counts(counts, ref.counts_ref(x, xp), f'knot edges counts {spacing} {env}')
    x32 = x.astype(np.float32)
    got, _, _ = run(x32, xp, fp, -9.0, 9.0)
    ref.same_bits(got, ref.curve_ref(x32, xp, fp, -9.0, 9.0), f'knot edges as float32 {spacing}')


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_workgroups_that_walk_several_spans(kind):
    """the plan's own choice on a grid large enough for it (two spans a workgroup: the last workgroup of a row has one),
    and forced choices on a short row: rows that end inside the first, a middle and the last span of a workgroup"""
    xs, fs = ref.ragged_batch()
    S = SPAN[kind]
    for spans in (2, 3, 16):
        for n in (S - 3, 2 * S + 1, 3 * S, 5 * S + 7):
            x = ref.rows_input(n, xs, 500 + n, NP_OF[kind])
            with switches(WFK_CURVE_SPANS=spans):
                st = distortion.CurveStage(xs, fs, n, dtype=NP_OF[kind])
                assert st.plan.spans == spans
                st.close()
                got, counts, _ = run(x, xs, fs)
                again, _, _ = run(x, xs, fs, in_place=True)
            ref.same_bits(got, ref.curve_ref(x, xs, fs), f'spans={spans} n={n} {kind}')
            same_counts(counts, ref.counts_ref(x, xs), f'spans={spans} n={n} {kind}')
            assert bits_equal(again, got)
    if kind == 'f64':
        rows, n = 128, 32 * S + 3
        xp, fp = ref.log_knots(1024)
        st = distortion.CurveStage(xp, fp, n, batch=rows)
        assert st.plan.spans == 2, st.plan.spans
        st.close()
        rng = np.random.default_rng(7)
        x = rng.uniform(-0.01, 1.01, (rows, n))
        got, counts, _ = run(x, xp, fp)
        ref.same_bits(got, ref.curve_ref(x, xp, fp), f'{rows} x {n}')
        same_counts(counts, ref.counts_ref(x, xp), f'{rows} x {n} counts')
        assert counts[:, :2].min() > 100


def test_no_fused_multiply_add():
    """the sensitive case equals the unfused referee and differs from an exact fused evaluation"""
    x, xp, fp = ref.sensitive_case()
    want = ref.curve_ref(x, xp, fp)
    fused = ref.fused_row(x[0], xp, fp)
    assert np.count_nonzero(fused != want[0]) >= x.size // 10
    for in_place in (False, True):
        got, counts, _ = run(x, xp, fp, in_place=in_place)
        ref.same_bits(got, want, f'sensitive case in_place={in_place}')
        assert np.count_nonzero(got[0] != fused) >= x.size // 10 and not counts.any()
    x32 = x.astype(np.float32)                            # widened, computed in double, rounded once
    got, _, _ = run(x32, xp, fp)
    ref.same_bits(got, ref.curve_ref(x32, xp, fp), 'sensitive case as float32')


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_in_place_equals_out_of_place(kind):
    xs, fs = all_curves()
    for n in (7, SPAN[kind] + 1, 10007):
        x = ref.rows_input(n, xs, 600 + n, NP_OF[kind])
        out, c_out, _ = run(x, xs, fs, np.nan, 3.0)
        inp, c_in, _ = run(x, xs, fs, np.nan, 3.0, in_place=True)
        ref.same_bits(inp, ref.curve_ref(x, xs, fs, np.nan, 3.0), f'in place n={n} {kind}')
        assert np.array_equal(np.isnan(inp), np.isnan(out)) and np.array_equal(c_in, c_out)
        ref.same_bits(inp, out, f'in place against out of place n={n} {kind}')


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', [5, 1024, 4100, 4101])
def test_row_windows(n, kind):
    """rows as windows at an odd element offset with row stride n + 37: out of place the guards of the output stay and
    the input holds; in place the guards stay"""
    dtype = NP_OF[kind]
    xs, fs = ref.ragged_batch()
    x = ref.rows_input(n, xs, 700 + n, dtype)
    want, want_counts = ref.curve_ref(x, xs, fs, -1.0, np.nan), ref.counts_ref(x, xs)
    st = distortion.CurveStage(xs, fs, n, left=-1.0, right=np.nan, dtype=dtype)
    src, dst = Window(3, n, dtype, x), Window(3, n, dtype)
    c = torch.full((3, 3), -1, dtype=torch.int64, device=dev())
    res = st.apply_torch(src.win, dst.win, c)
    assert res.data_ptr() == dst.ptr and tuple(res.shape) == (3, n)
    ref.same_bits(dst.host(), want, f'window n={n} {kind}')
    dst.assert_guards()
    src.assert_holds(x)
    same_counts(c.cpu().numpy(), want_counts, f'window counts n={n} {kind}')
    assert st.apply_torch(src.win, src.win).data_ptr() == src.ptr               # in place, in the window
    ref.same_bits(src.host(), want, f'window in place n={n} {kind}')
    src.assert_guards()
    # an input whose rows sit 16-byte aligned where the output's do not, and the other way round
    V = 16 // np.dtype(dtype).itemsize
    wide_in = torch.zeros((3, n + 3 * V), dtype=src.win.dtype, device=dev())
    wide_out = torch.zeros((3, n + 3 * V), dtype=src.win.dtype, device=dev())
    for a in range(V):
        for b in range(V):
            wide_in[:, a:a + n].copy_(torch.from_numpy(x))
            got = st.apply_torch(wide_in[:, a:a + n], wide_out[:, b:b + n])
            ref.same_bits(got.cpu().numpy(), want, f'offsets in={a} out={b} n={n} {kind}')
    st.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_stores_stay_inside_the_row(kind):
    """a sentinel-filled output at every lead into a 16-byte slot: [0, n) is overwritten and nothing else is"""
    dtype = NP_OF[kind]
    V = 16 // np.dtype(dtype).itemsize
    raw = torch.int64 if kind == 'f64' else torch.int32
    sentinel = 0x7FF8A5A5A5A5A5A5 if kind == 'f64' else 0x7FC5A5A5
    xs, fs = ref.ragged_batch()
    for n in (1, 3, V + 1, SPAN[kind] - 1, SPAN[kind] + V + 1):
        x = ref.rows_input(n, xs, 800 + n, dtype, specials=False)       # no NaN: a sentinel left inside would show
        x = np.clip(x, [[p[0]] for p in xs], [[p[-1]] for p in xs]).astype(dtype)
        want = ref.curve_ref(x, xs, fs)
        st = distortion.CurveStage(xs, fs, n, dtype=dtype)
        xd = torch.from_numpy(x).to(dev())
        for lead in range(V):
            out = torch.empty((3, n + 2 * V + 3), dtype=xd.dtype, device=dev())
            out.view(raw).fill_(sentinel)
            st.apply_torch(xd, out[:, lead:lead + n])
            bits = out.view(raw).cpu().numpy()
            assert np.all(bits[:, :lead] == sentinel) and np.all(bits[:, lead + n:] == sentinel), (n, lead)
            ref.same_bits(out[:, lead:lead + n].cpu().numpy(), want, f'stores n={n} lead={lead} {kind}')
            assert not np.isnan(want).any()
        st.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('side', ['in_place', 'far_in', 'far_out'])
def test_far_rows(side, kind):
    """rows more than 2^32 elements apart on either side give the bits of ordinary windows, and their guards stay"""
    dtype = NP_OF[kind]
    n = 2 * SPAN[kind] + 3
    xs, fs = ref.ragged_batch()
    xs, fs = xs[1:], fs[1:]
    x = ref.rows_input(n, xs, 900, dtype)
    want, want_counts = ref.curve_ref(x, xs, fs), ref.counts_ref(x, xs)
    st = distortion.CurveStage(xs, fs, n, dtype=dtype)
    try:
        src = FarWindow(n, dtype, x) if side in ('in_place', 'far_in') else Window(2, n, dtype, x)
        dst = src if side == 'in_place' else (FarWindow(n, dtype) if side == 'far_out' else Window(2, n, dtype))
        c = torch.full((2, 3), -5, dtype=torch.int64, device=dev())
        assert st.apply_torch(src.win, dst.win, c).data_ptr() == dst.ptr
        torch.cuda.synchronize()
        ref.same_bits(dst.host(), want, f'far rows {side} {kind}')
        dst.assert_guards()
        if src is not dst:
            src.assert_holds(x)
        same_counts(c.cpu().numpy(), want_counts, f'far rows counts {side} {kind}')
    finally:
        st.close()


def test_overlap_and_refused_tensors():
    n, rows = 256, 4
    xp, fp = ref.uniform_knots(16)
    st = distortion.CurveStage(xp, fp, n, batch=rows)
    buf = torch.zeros(2 * rows * n + 64, dtype=torch.float64, device=dev())
    x = buf[:rows * n].view(rows, n)
    out = torch.zeros((rows, n), dtype=torch.float64, device=dev())
    counts = torch.zeros((rows, 3), dtype=torch.int64, device=dev())
    st.apply_torch(x, out, counts)                                               # fine
    st.apply_torch(x, x, counts)                                                 # in place: fine
    st.apply_torch(x, buf[rows * n:2 * rows * n].view(rows, n), counts)          # adjacent: fine
    for bad_out in (buf[8:8 + rows * n].view(rows, n), buf[rows * n - 1:2 * rows * n - 1].view(rows, n),
                    buf[:rows * (n + 2)].view(rows, n + 2)[:, :n]):               # the same start, another stride
        with pytest.raises(ValueError, match='overlaps'):
            st.apply_torch(x, bad_out, counts)
    over_x = buf[8:8 + rows * 3].view(torch.int64).view(rows, 3)
    over_out = out.view(-1)[16:16 + rows * 3].view(torch.int64).view(rows, 3)
    for bad_counts in (over_x, over_out):
        with pytest.raises(ValueError, match='counts overlaps'):
            st.apply_torch(x, out, bad_counts)
    with pytest.raises(ValueError, match='counts overlaps'):
        st.apply_torch(x, x, over_x)
    wide = torch.zeros((rows, 4), dtype=torch.int64, device=dev())
    for bad_counts in (counts[:3], counts.view(-1), wide[:, :3], counts.to(torch.int32), counts.to(torch.float64),
                       counts.cpu(), torch.zeros((rows, 2), dtype=torch.int64, device=dev())):
        with pytest.raises(ValueError, match='counts'):
            st.apply_torch(x, out, bad_counts)
    xc = torch.zeros((rows, n), dtype=torch.float64, device=dev())
    for bad in (xc[:2], xc[:, :n - 1], xc.to(torch.float32), xc.cpu(), xc.t().contiguous().t(), xc.view(2, rows // 2, n)):
        with pytest.raises(ValueError, match='expected x'):
            st.apply_torch(bad, out)
        with pytest.raises(ValueError, match='expected out'):
            st.apply_torch(xc, bad)
    st.close()
    empty = distortion.CurveStage(xp, fp, 0, batch=2)                            # n = 0: a no-op that zeroes the counts
    e = torch.zeros((2, 0), dtype=torch.float64, device=dev())
    c = torch.full((2, 3), 5, dtype=torch.int64, device=dev())
    assert tuple(empty.apply_torch(e, counts=c).shape) == (2, 0)
    assert not c.cpu().numpy().any()
    empty.close()


def test_library_refuses_a_bad_apply():
    """the C side's own checks of an apply, through the raw pointers, one case per clause of the row rule; nothing is
    launched.  n = 0: a no-op that zeroes the report, whatever the row pointers"""
    rows, n = 4, 40
    xp, fp = ref.uniform_knots(16)
    st = distortion.CurveStage(xp, fp, n, batch=rows)
    x = torch.ones((rows + 1, n), dtype=torch.float64, device=dev())
    out = torch.full((rows, n), 123.0, dtype=torch.float64, device=dev())
    counts = torch.full((rows, 3), 7, dtype=torch.int64, device=dev())
    lib, h = _engine.lib(), st.plan._h
    X, Y, Cn = x.data_ptr(), out.data_ptr(), counts.data_ptr()
    for args, message in (((None, n, Y, n, None), b'null in / out'),
                          ((X, n, None, n, None), b'null in / out'),
                          ((X + 4, n, Y, n, None), b'not aligned to their element'),
                          ((X, n, Y + 2, n, None), b'not aligned to their element'),
                          ((X, n - 1, Y, n, None), b'in row stride smaller'),
                          ((X, n, Y, n - 1, None), b'out row stride smaller'),
                          ((X, n, X + 8, n, None), b'curve rows is out of place: out overlaps in'),
                          ((X + 8 * n, n, X, n, None), b'out overlaps in'),
                          ((X, n + 1, X, n, None), b'out overlaps in'),                       # the same start, other strides
                          ((X, n, Y, n, Cn + 4), b'counts are not aligned'),
                          ((X, n, Y, n, X + 16), b'counts overlaps in'),
                          ((X, n, Y, n, Y + 8), b'counts overlaps out'),
                          ((X, n, X, n, X + 16), b'counts overlaps in')):
        assert lib.wfk_curve_rows_apply(h, *args, None) == -1, args
        text = lib.wfk_last_error()
        assert text.startswith(b'curve rows') and message in text, (args, text)
        with pytest.raises(_engine.EngineError, match=message.decode()):
            st.apply(*args)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 123.0) and np.all(counts.cpu().numpy() == 7) and np.all(x.cpu().numpy() == 1.0)
    st.close()
    empty = distortion.CurveStage(xp, fp, 0, batch=rows)
    assert lib.wfk_curve_rows_apply(empty.plan._h, None, 0, None, 0, Cn, None) == 0
    torch.cuda.synchronize()
    assert not counts.cpu().numpy().any()
    assert lib.wfk_curve_rows_apply(empty.plan._h, None, 0, None, 0, None, None) == 0
    assert lib.wfk_curve_rows_apply(empty.plan._h, None, 0, None, 0, Cn + 4, None) == -1
    assert b'counts are not aligned' in lib.wfk_last_error()
    empty.close()


def test_side_stream_equals_default_stream():
    n = 4099
    xs, fs = ref.ragged_batch()
    x = ref.rows_input(n, xs, 1000)
    st = distortion.CurveStage(xs, fs, n)
    xd = torch.from_numpy(x).to(dev())
    ca = torch.empty((3, 3), dtype=torch.int64, device=dev())
    a = st.apply_torch(xd, counts=ca).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z = torch.from_numpy(x).to(dev())
        cb = torch.full((3, 3), 99, dtype=torch.int64, device=dev())
        b = st.apply_torch(z, counts=cb).clone()                  # produced and consumed on the side stream
        cb = cb + 0
    side.synchronize()
    want = ref.curve_ref(x, xs, fs)
    ref.same_bits(a, want, 'default stream')
    ref.same_bits(b.cpu().numpy(), want, 'side stream')
    same_counts(ca.cpu().numpy(), ref.counts_ref(x, xs), 'default stream, counts')
    same_counts(cb.cpu().numpy(), ref.counts_ref(x, xs), 'side stream, counts')
    st.close()


@pytest.mark.parametrize('kind,in_place', [('f64', False), ('f32', True)])
def test_graph_replay(kind, in_place):
    """one apply with counts captured and replayed on A, B, A: each replay gives the bits and the counts of the referee
    and of an eager twin plan, and leaves no sentinel inside the rows (no input holds a NaN here)"""
    dtype = NP_OF[kind]
    n = 4099
    xs, fs = ref.ragged_batch()
    feeds = []
    for seed in (1100, 1101):
        x = ref.rows_input(n, xs, seed, dtype, specials=False)
        x[:, ::97] = np.inf                                       # some of every count but nan
        x[:, 5::89] = -np.inf
        feeds.append(x)
    assert not np.array_equal(ref.counts_ref(feeds[0], xs), ref.counts_ref(feeds[1], xs))

    def make():
        st = distortion.CurveStage(xs, fs, n, dtype=dtype)
        x = torch.empty((3, n), dtype=torch.float64 if kind == 'f64' else torch.float32, device=dev())
        out = x if in_place else torch.empty_like(x)
        counts = torch.empty((3, 3), dtype=torch.int64, device=dev())
        return st, (lambda: st.apply_torch(x, out, counts)), [x], [out, counts]

    st, run_, statics, outputs = make()
    twin, trun, tstatics, toutputs = make()
    assert st.kernel_name(counts=True) == f'curve_rows_counts<{NAME_OF[kind]}>'
    got = replay(run_, statics, [(feeds[0], ), (feeds[1], ), (feeds[0], )], outputs)
    for k, (y, counts) in enumerate(got):
        x = feeds[k % 2]
        ref.same_bits(y, ref.curve_ref(x, xs, fs), f'replay {k} {kind}')
        same_counts(counts, ref.counts_ref(x, xs), f'replay {k} counts {kind}')
        ty, tcounts = eager(trun, tstatics, (x, ), toutputs)
        assert bits_equal(y, ty) and np.array_equal(counts, tcounts), k
        assert sentinels_left(y) == 0 and sentinels_left(counts) == 0, k
    st.close()
    twin.close()


def test_numpy_round_trip():
    xs, fs = ref.ragged_batch()
    x = ref.rows_input(3001, xs, 1200)
    want, want_counts = ref.curve_ref(x, xs, fs, 0.25, np.nan), ref.counts_ref(x, xs)
    ref.same_bits(distortion.interp_rows(x, xs, fs, 0.25, np.nan), want, 'interp_rows')
    y, counts = distortion.interp_rows(x, xs, fs, 0.25, np.nan, return_counts=True)
    ref.same_bits(y, want, 'interp_rows with counts')
    same_counts(counts, want_counts, 'interp_rows counts')
    x32 = x.astype(np.float32)
    y32 = distortion.interp_rows(x32, xs, fs)
    assert y32.dtype == np.float32
    ref.same_bits(y32, ref.curve_ref(x32, xs, fs), 'float32 rows')
    xp, fp = np.array([-100.0, 0.0, 50.0, 100.0]), np.array([1.0, 0.5, 0.75, -2.0])
    xi = np.random.default_rng(3).integers(-120, 120, (2, 500)).astype(np.int32)
    yi = distortion.interp_rows(xi, xp, fp)                                       # integers are read as float64
    assert yi.dtype == np.float64
    ref.same_bits(yi, ref.curve_ref(xi.astype(np.float64), xp, fp), 'integer input, one shared curve')
    for r in range(2):
        assert np.array_equal(yi[r], np.interp(xi[r], xp, fp))


def test_pipeline_detuning_to_volts_to_codes():
    """BatchSampler rows (detuning) -> CurveStage.inverse of the measured f(V) (volts) -> IirStage -> DacStage, against
    the referee chain stage by stage: the curve and the codes bit for bit from what the device fed them, the IIR against
    SciPy at the suite's IIR bound"""
    from scipy.signal import lfilter
    from waveforms_amd import cos
    from waveforms_amd._sampling import BatchSampler
    rows, n = 4, 4099
    chans = [0.3 * cos(2 * np.pi * 50e6, 0.1 * s) + 0.1 * cos(2 * np.pi * 125e6) for s in range(rows)]
    x = BatchSampler(chans, ('linspace', 0.0, n * 1e-9, n, False)).launch_torch(
        torch.empty((rows, n), dtype=torch.float64, device=dev()))
    detuning = x.cpu().numpy()
    volts = np.linspace(-1.0, 1.0, 129)
    measured = [(0.25 + 0.02 * r) * volts + 0.08 * volts**3 for r in range(rows)]       # f(V), monotone, per line
    measured[1] = -measured[1]                                                           # a line wired the other way round
    curve = distortion.CurveStage.inverse([volts] * rows, measured, n)
    inv_x, inv_f = distortion.CurveStage.inverse_rows([volts] * rows, measured)
    counts = torch.empty((rows, 3), dtype=torch.int64, device=dev())
    v = curve.apply_torch(x, counts=counts)
    ref.same_bits(v.cpu().numpy(), ref.curve_ref(detuning, inv_x, inv_f), 'detuning to volts')
    same_counts(counts.cpu().numpy(), ref.counts_ref(detuning, inv_x), 'samples beyond the measured range')
    assert counts.cpu().numpy()[0, :2].min() > 0 and not counts.cpu().numpy()[:, 2].any()   # |x| reaches 0.4 > f(1) of line 0
    assert np.max(np.abs(v.cpu().numpy())) <= 1.0
    secs = [[distortion.exp_decay_filter(0.02 + 0.01 * r, 150e-9, 1e9)] for r in range(rows)]
    iir = distortion.IirStage(secs, n, rows)
    vd = v.cpu().numpy()
    y = iir.apply_torch(v.clone())
    yd = y.cpu().numpy()
    for r in range(rows):
        b, a = secs[r][0]
        want = lfilter(b, a, vd[r])
        assert np.max(np.abs(yd[r] - want)) <= FP64_IIR_TOL * max(1.0, np.abs(want).max()), r
    dac = distortion.DacStage.from_full_scale(1.25, n, batch=rows)
    codes = dac.apply_torch(y).cpu().numpy()
    want_codes, _ = dac_rows_ref.dac_ref(yd, dac.gain, dac.offset)
    assert np.array_equal(codes, want_codes) and len(np.unique(codes)) > 100       # (the rows are periodic: 40 ns)
    for st in (curve, iir, dac):
        st.close()


def test_plain_c_consumer_interpolates_on_the_device(tmp_path):
    exe = tmp_path / 'curve_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'curve_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert '16 values interpolated on the device, parity ok' in r.stdout, r.stdout
