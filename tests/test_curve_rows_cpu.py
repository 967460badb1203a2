"""The curve stage (distortion.CurveStage / interp_rows), everything up to the point a device is needed: the referee
(tests/curve_rows_ref.py) held to np.interp bit for bit, the contraction-sensitive case held to exact rational arithmetic,
the argument checks that come before any device work, and the declarations of the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import curve_rows_ref as ref
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _interp_rows(x, xs, fs, left, right):
    return np.stack([np.interp(x[r].astype(np.float64), xs[r], fs[r], left[r], right[r]).astype(x.dtype)
                     for r in range(len(xs))])


@pytest.mark.parametrize('spacing', ['uniform', 'log'])
@pytest.mark.parametrize('K', [2, 3, 64, 65, 1023, 1024])
def test_referee_is_np_interp_bit_for_bit(K, spacing):
    """rows shorter than K (NumPy's path without precomputed slopes) and longer (with them), the builders' specials in them,
    default and explicit ends, NaN ends among them"""
    xp, fp = ref.knots(K, spacing)
    for n in (1, K // 2 + 1, K, 4 * K + 3, 3 * K + 7 + 5):
        x = np.stack([ref.row_input(n, xp, 10 + n), np.resize(np.concatenate([ref.knot_edges(xp), [np.nan, np.inf, -np.inf, 0.0, -0.0]]), n)])
        for left, right in ((None, None), ([7.5, np.nan], [np.nan, -2.25])):
            got = ref.curve_ref(x, xp, fp, left, right)
            l = [fp[0]] * 2 if left is None else left
            r = [fp[-1]] * 2 if right is None else right
            ref.same_bits(got, _interp_rows(x, [xp] * 2, [fp] * 2, l, r), f'K={K} {spacing} n={n} ends={left}')
    x32 = ref.row_input(4 * K + 1, xp, 3, np.float32)[None]
    ref.same_bits(ref.curve_ref(x32, xp, fp), _interp_rows(x32, [xp], [fp], [fp[0]], [fp[-1]]), f'float32 K={K} {spacing}')


def test_referee_on_a_ragged_batch_and_its_counts():
    xs, fs = ref.ragged_batch()
    assert [len(x) for x in xs] == [2, 1024, 65]
    x = ref.rows_input(5000, xs, 40)
    got = ref.curve_ref(x, xs, fs)
    ref.same_bits(got, _interp_rows(x, xs, fs, [f[0] for f in fs], [f[-1] for f in fs]), 'ragged')
    counts = ref.counts_ref(x, xs)
    assert counts.dtype == np.int64 and counts.shape == (3, 3) and counts.min() >= 1
    for r in range(3):
        assert counts[r].tolist() == [int(np.sum(x[r] < xs[r][0])), int(np.sum(x[r] > xs[r][-1])), int(np.sum(np.isnan(x[r])))]
        assert np.count_nonzero(np.isnan(got[r])) == counts[r, 2]
    # -0.0 at a knot that is 0.0 takes the knot's value; -inf / +inf count as below / above; a NaN stays
    one = ref.curve_ref(np.array([[-0.0, 0.0, -np.inf, np.inf, np.nan]]), np.array([0.0, 1.0]), np.array([-0.0, 5.0]), 8.0, 9.0)
    assert one.tolist()[0][:4] == [0.0, 0.0, 8.0, 9.0] and np.isnan(one[0, 4])
    assert np.signbit(one[0, :2]).tolist() == [True, True]
    assert ref.counts_ref(np.array([[-0.0, 0.0, -np.inf, np.inf, np.nan]]), np.array([0.0, 1.0])).tolist() == [[1, 1, 1]]


def test_same_bits_sees_a_sign_a_payload_free_nan_and_a_last_bit():
    a = np.array([[0.0, 1.0, np.nan]])
    ref.same_bits(a, a.copy(), 'equal')
    for bad in (np.array([[-0.0, 1.0, np.nan]]), np.array([[0.0, np.nextafter(1.0, 2.0), np.nan]]),
                np.array([[0.0, 1.0, 0.0]]), np.array([[0.0, np.nan, np.nan]])):
        with pytest.raises(AssertionError, match='differ'):
            ref.same_bits(bad, a, 'x')


def test_sensitive_case_changes_under_a_fused_multiply_add():
    """an exact fused evaluation of the last two operations changes at least 10 % of the samples"""
    x, xp, fp = ref.sensitive_case()
    want = ref.curve_ref(x, xp, fp)
    ref.same_bits(want, np.interp(x[0], xp, fp)[None], 'sensitive case against np.interp')
    fused = ref.fused_row(x[0], xp, fp)
    changed = np.count_nonzero(fused != want[0])
    print(f'{changed} of {x.size} samples change under a fused multiply-add')
    assert changed >= x.size // 10
    # (the two differ by the rounding of the product, at most half an ulp of a product below 4, and one of the sum)
    assert np.max(np.abs(fused - want[0])) <= 2.0**-51


def test_arguments_layout_dtypes_and_broadcasting():
    xs, fs = ref.ragged_batch()
    ptr, xp, fp, left, right, n, dtype = _engine.curve_rows_arguments(xs, fs, None, None, None, 100, np.float32)
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 2, 1026, 1091]
    assert xp.dtype == fp.dtype == left.dtype == right.dtype == np.float64 and xp.flags.c_contiguous
    assert np.array_equal(xp, np.concatenate(xs)) and np.array_equal(fp, np.concatenate(fs))
    assert left.tolist() == [f[0] for f in fs] and right.tolist() == [f[-1] for f in fs]
    assert (n, dtype) == (100, np.dtype(np.float32))
    # a 2-D array: one curve per row; explicit ends, a scalar and one per row, NaN allowed
    x2, f2 = np.array([[0.0, 1.0, 2.0], [5.0, 6.0, 7.0]]), np.array([[1, 2, 3], [9, 8, 7]])
    ptr, xp, fp, left, right, _, _ = _engine.curve_rows_arguments(x2, f2, np.nan, [1.5, -np.inf], None, 0, np.float64)
    assert ptr.tolist() == [0, 3, 6] and fp.tolist() == [1.0, 2.0, 3.0, 9.0, 8.0, 7.0]
    assert np.isnan(left).all() and right.tolist() == [1.5, -np.inf]
    # one 1-D pair for `batch` rows (lists of scalars too)
    for pair in ((x2[0], f2[0]), ([0.0, 1.0, 2.0], [1, 2, 3])):
        ptr, xp, fp, left, right, _, _ = _engine.curve_rows_arguments(pair[0], pair[1], None, None, 4, 8, np.float64)
        assert ptr.tolist() == [0, 3, 6, 9, 12] and xp.tolist() == [0.0, 1.0, 2.0] * 4 and fp.tolist() == [1.0, 2.0, 3.0] * 4
        assert left.tolist() == [1.0] * 4 and right.tolist() == [3.0] * 4
    assert _engine.curve_rows_arguments(x2[0], f2[0], None, None, None, 8, np.float64)[0].tolist() == [0, 3]


def test_arguments_refuse_with_the_row_named():
    ok_x, ok_f = np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0, 4.0])
    big = np.arange(_engine.CURVE_MAX_KNOTS + 1, dtype=np.float64)

    def args(xs, fs, left=None, right=None, batch=None, n=16, dtype=np.float64):
        return _engine.curve_rows_arguments(xs, fs, left, right, batch, n, dtype)

    for xs, fs, kw, message in (
            ([ok_x, [1.0]], [ok_f, [1.0]], {}, 'row 1: fewer than 2 knots'),
            ([ok_x, ok_x, big], [ok_f, ok_f, big], {}, 'row 2: more than 1024 knots'),
            ([ok_x, [0.0, 1.0, 1.0]], [ok_f, ok_f], {}, 'row 1: knots are not strictly increasing at 2'),
            ([[0.0, 2.0, 1.0, 3.0]], [[0.0, 0.0, 0.0, 0.0]], {}, 'row 0: knots are not strictly increasing at 2'),
            ([ok_x, [0.0, np.nan, 2.0]], [ok_f, ok_f], {}, 'row 1: knot 1 is not finite'),
            ([[0.0, 1.0, np.inf]], [ok_f], {}, 'row 0: knot 2 is not finite'),
            ([[-np.inf, 1.0, 2.0]], [ok_f], {}, 'row 0: knot 0 is not finite'),
            ([ok_x, ok_x], [ok_f, [0.0, np.inf, 1.0]], {}, 'row 1: value 1 is not finite'),
            ([ok_x], [[np.nan, 0.0, 1.0]], {}, 'row 0: value 0 is not finite'),
            ([ok_x, ok_x], [ok_f, [0.0, 1.0]], {}, 'row 1: 3 knots and 2 values'),
            ([ok_x, ok_x], [ok_f], {}, '2 rows of xp and 1 rows of fp'),
            ([ok_x, ok_x], [ok_f, ok_f], {'batch': 3}, '2 curves for 3 rows'),
            ([], [], {}, 'no rows'),
            (ok_x, ok_f, {'batch': 0}, 'no rows'),
            (ok_x, ok_f, {'n': -1}, 'n >= 0'),
            (ok_x, ok_f, {'dtype': np.int16}, 'dtype must be float64 or float32'),
            (ok_x, ok_f, {'batch': 2, 'left': [1.0, 2.0, 3.0]}, '3 values of left for 2 rows'),
            (ok_x, ok_f, {'batch': 2, 'right': [1.0]}, '1 values of right for 2 rows'),
            (np.zeros((2, 2, 2)), np.zeros((2, 2, 2)), {}, 'xp: a list of 1-D arrays'),
            ([np.zeros((2, 2)), ok_x], [ok_f, ok_f], {}, 'row 0: xp is not 1-D')):
        with pytest.raises(ValueError, match=re.escape(message)):
            args(xs, fs, **kw)
        if 'batch' not in kw and 'left' not in kw and 'right' not in kw:
            with pytest.raises(ValueError, match=re.escape(message)):
                distortion.CurveStage(xs, fs, kw.get('n', 16), dtype=kw.get('dtype', np.float64))
    with pytest.raises(NotImplementedError):
        args(ok_x, ok_f, dtype=np.complex128)
    with pytest.raises(NotImplementedError):
        args([ok_x + 0j], [ok_f])
    # any double is a legal end
    assert np.isnan(args(ok_x, ok_f, left=np.nan, right=np.inf)[3][0])


def test_inverse_swaps_reverses_and_refuses():
    v = np.array([-1.0, 0.0, 0.5, 2.0])
    up, down = np.array([10.0, 11.0, 15.0, 16.0]), np.array([3.0, 2.5, 1.0, -4.0])
    nx, nf = distortion.CurveStage.inverse_rows([v, v], [up, down])
    assert nx[0].tolist() == up.tolist() and nf[0].tolist() == v.tolist()
    assert nx[1].tolist() == down[::-1].tolist() and nf[1].tolist() == v[::-1].tolist()
    for r in range(2):                                             # the round trip at the measured points
        f = (up, down)[r]
        back = ref.curve_ref(f[None], [nx[r]], [nf[r]])
        assert np.array_equal(back[0], v)
    nx, nf = distortion.CurveStage.inverse_rows(v, down)           # one 1-D pair
    assert len(nx) == 1 and nx[0].tolist() == down[::-1].tolist()
    for bad, row in (([up, np.array([1.0, 2.0, 2.0, 3.0])], 1), ([np.array([1.0, 3.0, 2.0, 4.0]), down], 0),
                     ([up, np.array([1.0, np.nan, 3.0, 4.0])], 1)):
        with pytest.raises(ValueError, match=f'row {row}: values are not strictly monotone'):
            distortion.CurveStage.inverse_rows([v, v], bad)
        with pytest.raises(ValueError, match=f'row {row}: values are not strictly monotone'):
            distortion.CurveStage.inverse([v, v], bad, 64)
    with pytest.raises(ValueError, match='row 1: 4 knots and 3 values'):
        distortion.CurveStage.inverse_rows([v, v], [up, down[:3]])
    with pytest.raises(ValueError, match='row 0: value 1 is not finite'):                 # the measured points become values
        distortion.CurveStage.inverse([np.array([0.0, np.inf, 1.0, 2.0])], [up], 64)


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_curve_rows_plan_create', 'wfk_curve_rows_apply', 'wfk_curve_rows_plan_destroy',
                 'wfk_curve_rows_kernel_name', 'wfk_curve_rows_spans'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_curve_rows_plan wfk_curve_rows_plan;' in src
    m = re.search(r'#define\s+WFK_CURVE_MAX_KNOTS\s+(\d+)', src)
    assert m and int(m.group(1)) == _engine.CURVE_MAX_KNOTS == ref.MAX_KNOTS == 1024
    assert lib.wfk_abi_version() == 2
    assert re.search(r'#define\s+WFK_ABI_VERSION\s+2\b', src)


def test_library_refuses_before_any_device_work():
    """the C side's own refusals come before it looks for a device: WFK_EINVAL (-1) here, with the row named"""
    lib = _engine.lib()
    create = lib.wfk_curve_rows_plan_create
    h = C.c_void_p()

    def call(n, batch, kind, ptr, xp, fp, left=None, right=None):
        p = (C.c_int64 * len(ptr))(*ptr) if ptr is not None else None
        x = (C.c_double * len(xp))(*xp) if xp is not None else None
        f = (C.c_double * len(fp))(*fp) if fp is not None else None
        rc = create(n, batch, kind, p, x, f, left, right, C.byref(h))
        assert not h
        return rc, lib.wfk_last_error()

    ok_x, ok_f = [0.0, 1.0, 2.0, 5.0, 6.0], [0.0, 1.0, 4.0, 1.0, 2.0]
    for a, message in (((-1, 2, 0, [0, 3, 5], ok_x, ok_f), b'bad curve rows plan arguments'),
                       ((64, 0, 0, [0, 3, 5], ok_x, ok_f), b'bad curve rows plan arguments'),
                       ((64, 2, 0, None, ok_x, ok_f), b'bad curve rows plan arguments'),
                       ((64, 2, 0, [0, 3, 5], None, ok_f), b'bad curve rows plan arguments'),
                       ((64, 2, 0, [0, 3, 5], ok_x, None), b'bad curve rows plan arguments'),
                       ((64, 2, 2, [0, 3, 5], ok_x, ok_f), b'kind must be F64 or F32'),
                       ((64, 2, 0, [1, 3, 5], ok_x, ok_f), b'knot_ptr is not non-decreasing from 0'),
                       ((64, 2, 0, [0, 3, 2], ok_x, ok_f), b'knot_ptr is not non-decreasing from 0'),
                       ((64, 2, 0, [0, 4, 5], ok_x, ok_f), b'row 1: fewer than 2 knots'),
                       ((64, 2, 0, [0, 0, 5], ok_x, ok_f), b'row 0: fewer than 2 knots'),
                       ((64, 1, 0, [0, 1025], list(range(1025)), [0.0] * 1025), b'row 0: more than 1024 knots'),
                       ((64, 2, 0, [0, 3, 5], [0.0, 1.0, 2.0, 6.0, 6.0], ok_f), b'row 1: knots are not strictly increasing at 1'),
                       ((64, 2, 0, [0, 3, 5], [0.0, 2.0, 1.0, 5.0, 6.0], ok_f), b'row 0: knots are not strictly increasing at 2'),
                       ((64, 2, 0, [0, 3, 5], [0.0, 1.0, float('inf'), 5.0, 6.0], ok_f), b'row 0: knot 2 is not finite'),
                       ((64, 2, 0, [0, 3, 5], [0.0, 1.0, 2.0, float('nan'), 6.0], ok_f), b'row 1: knot 0 is not finite'),
                       ((64, 2, 0, [0, 3, 5], ok_x, [0.0, 1.0, 4.0, 1.0, float('nan')]), b'row 1: value 1 is not finite'),
                       ((2**62, 2, 0, [0, 3, 5], ok_x, ok_f), b'batch * n too large for one launch')):
        rc, text = call(*a)
        assert rc == -1 and message in text, (a[:4], rc, text)
    assert create(64, 2, 0, (C.c_int64 * 3)(0, 3, 5), (C.c_double * 5)(*ok_x), (C.c_double * 5)(*ok_f), None, None, None) == -1
    assert lib.wfk_curve_rows_apply(None, None, 64, None, 64, None, None) == -1
    assert b'null plan' in lib.wfk_last_error()
    assert lib.wfk_curve_rows_plan_destroy(None) == 0
    assert lib.wfk_curve_rows_kernel_name(None, 0) == b'' and lib.wfk_curve_rows_kernel_name(None, 1) == b''
    assert lib.wfk_curve_rows_spans(None) == 0


def test_interp_rows_refuses_and_answers_empty_rows_without_a_device():
    xp, fp = np.array([0.0, 1.0]), np.array([2.0, 3.0])
    with pytest.raises(ValueError, match='2-D'):
        distortion.interp_rows(np.zeros(16), xp, fp)
    with pytest.raises(ValueError, match='2-D'):
        distortion.interp_rows(np.zeros((2, 2, 4)), xp, fp)
    with pytest.raises(NotImplementedError):
        distortion.interp_rows(np.zeros((2, 4)) + 0j, xp, fp)
    with pytest.raises(ValueError, match='2 curves for 3 rows'):
        distortion.interp_rows(np.zeros((3, 4)), [xp, xp], [fp, fp])
    with pytest.raises(ValueError, match='row 1: knots are not strictly increasing at 1'):
        distortion.interp_rows(np.zeros((2, 4)), [xp, xp[::-1]], [fp, fp])
    with pytest.raises(ValueError, match='no rows'):
        distortion.interp_rows(np.zeros((0, 4)), xp, fp)
    y, counts = distortion.interp_rows(np.zeros((2, 0), dtype=np.float32), xp, fp, return_counts=True)
    assert y.shape == (2, 0) and y.dtype == np.float32
    assert counts.shape == (2, 3) and counts.dtype == np.int64 and not counts.any()
    y = distortion.interp_rows(np.zeros((3, 0), dtype=np.int32), xp, fp)
    assert y.shape == (3, 0) and y.dtype == np.float64
    with pytest.raises(ValueError, match='row 0: fewer than 2 knots'):
        distortion.interp_rows(np.zeros((2, 0)), [1.0], [1.0])
