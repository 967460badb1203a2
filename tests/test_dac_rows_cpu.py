"""The DAC stage (distortion.DacStage / dac_codes_rows), everything up to the point a device is needed: the referee's
own properties (tests/dac_rows_ref.py), the builder of rounding-sensitive rows held to exact rational arithmetic, the
argument checks that come before any device work, and the declarations of the header."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dac_rows_ref as ref
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_referee_rounds_half_to_even_in_both_signs():
    x = np.array([[0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 0.49999999999999994, -0.0, 0.0]])
    codes, counts = ref.dac_ref(x, 1.0)
    assert codes.tolist() == [[0, 2, 2, 4, 0, -2, -2, -4, 0, 0, 0]]
    assert codes.dtype == np.int16 and counts.dtype == np.int64 and not counts.any()
    codes, _ = ref.dac_ref(x.astype(np.float32)[:, :8], 1.0)
    assert codes.tolist() == [[0, 2, 2, 4, 0, -2, -2, -4]]


def test_referee_rails_infinities_and_nan():
    for bits in (16, 14, 12, 2):
        lo, hi = ref.rails(bits)
        assert (lo, hi) == (-2**(bits - 1), 2**(bits - 1) - 1)
        x = np.array([[lo, lo - 0.5, lo - 0.5000001, lo - 1, hi, hi + 0.5, hi + 0.4999999, hi + 1, np.inf, -np.inf,
                       np.nan, 0.0]], dtype=np.float64)
        codes, counts = ref.dac_ref(x, 1.0, bits=bits)
        # lo - 0.5 ties to the even lo (in range); hi + 0.5 ties to the even hi + 1 (clipped)
        assert codes.tolist() == [[lo, lo, lo, lo, hi, hi, hi, hi, hi, lo, 0, 0]], bits
        assert counts.tolist() == [[3, 3, 1]], bits
    # inf * 0 and inf - inf are NaN: code 0, counted as nan and nowhere else
    codes, counts = ref.dac_ref(np.array([[np.inf, 1.0]]), 0.0, offset=3.0)
    assert codes.tolist() == [[0, 3]] and counts.tolist() == [[0, 0, 1]]
    # a negative gain swaps the rails
    codes, counts = ref.dac_ref(np.array([[1e9, -1e9]]), -1.0, bits=12)
    assert codes.tolist() == [[-2048, 2047]] and counts.tolist() == [[1, 1, 0]]


def test_referee_shift_leaves_the_low_bits_zero():
    x = np.random.default_rng(0).uniform(-40000, 40000, (3, 500))
    for bits, shift in ((14, 2), (12, 4), (12, 0), (2, 14), (15, 1)):
        plain, c0 = ref.dac_ref(x, 1.0, bits=bits)
        codes, c1 = ref.dac_ref(x, 1.0, bits=bits, shift=shift)
        assert not np.any(codes.astype(np.int32) & (2**shift - 1))
        assert np.array_equal(codes.astype(np.int32) >> shift, plain) and np.array_equal(c0, c1)
        assert codes.min() == -2**(bits - 1) * 2**shift and codes.max() == (2**(bits - 1) - 1) * 2**shift


def test_referee_interleave_layout_and_per_row_counts():
    rng = np.random.default_rng(1)
    x = rng.uniform(-40000, 40000, (6, 37))
    g, o = rng.uniform(0.5, 1.5, 6) * [1, -1, 1, 1, -1, 1], rng.uniform(-100, 100, 6)
    one, c1 = ref.dac_ref(x, g, o)
    two, c2 = ref.dac_ref(x, g, o, interleave=2)
    assert one.shape == (6, 37) and two.shape == (3, 74) and np.array_equal(c1, c2) and c1.shape == (6, 3)
    for r in range(3):
        assert np.array_equal(two[r, 0::2], one[2 * r]) and np.array_equal(two[r, 1::2], one[2 * r + 1])
    assert c1[:, :2].sum() > 0


def test_sensitive_rows_are_exact_ties_that_a_fused_multiply_add_or_half_away_breaks():
    g, M = 9731.37, 20000
    x, ks = ref.sensitive_row(1024, g, M, seed=7)
    assert len(x) == 1024
    fused_differs = away_differs = 0
    for xi, k in zip(x, ks):
        k = int(k)
        exact = Fraction(float(xi)) * Fraction(g)
        assert float(exact) == M + k + 0.5                       # the rounded product is the tie ...
        assert (M + k + 0.5) - M == k + 0.5                        # ... and the rounded sum keeps it
        tie_code = int(np.rint(k + 0.5))
        assert tie_code == (k if k % 2 == 0 else k + 1)
        fused = ref.fused_value(xi, g, M)
        assert fused == float(exact - M)
        assert abs(fused - (k + 0.5)) <= 2.0**-39                  # off the tie by the product's rounding error at most
        fused_differs += int(np.rint(fused)) != tie_code
        away_differs += int(ref.half_away(k + 0.5)) != tie_code
    print(f'1024 ties, {fused_differs} fused-sensitive, {away_differs} half-away-sensitive')
    assert fused_differs >= 256 and away_differs >= 256
    codes, counts = ref.dac_ref(x[None, :], g, -float(M))
    assert np.array_equal(codes[0], np.rint(ks + 0.5).astype(np.int16)) and not counts.any()


def test_float32_tie_rows_are_exact_ties():
    x, ks, gain = ref.tie_row32()
    assert x.dtype == np.float32 and len(x) == 1024
    for xi, k in zip(x[:64], ks[:64]):
        assert Fraction(float(xi)) * Fraction(gain) == Fraction(2 * int(k) + 1, 2)
    codes, counts = ref.dac_ref(x[None, :], gain, 7.0)
    want = np.rint(ks + 7.5)
    assert np.array_equal(codes[0], want.astype(np.int16)) and not counts.any()
    assert np.count_nonzero(ref.half_away(ks + 7.5) != want) >= 256


def test_from_full_scale_maps_full_scale_to_hi():
    for bits in (16, 14, 12):
        hi = 2**(bits - 1) - 1
        for fs in (1.0, 0.35, 2.5):
            gain = hi / fs
            codes, counts = ref.dac_ref(np.array([[fs, -fs, 0.0]]), gain, bits=bits)
            assert codes.tolist() == [[hi, -hi, 0]] and not counts.any()
    for bad in (0.0, -1.0, np.inf, np.nan, [1.0, 0.0], [1.0, np.nan]):
        with pytest.raises(ValueError, match='full scale'):
            distortion.DacStage.from_full_scale(bad, 64, batch=2)
    with pytest.raises(ValueError, match='bits'):
        distortion.DacStage.from_full_scale(1.0, 64, batch=2, bits=17)


def test_stage_refuses_before_any_device_work():
    with pytest.raises(ValueError, match='batch'):
        distortion.DacStage(1000.0, 64)                                            # scalars need batch=
    with pytest.raises(ValueError, match='batch'):
        distortion.DacStage(1000.0, 64, offset=3.0)
    with pytest.raises(ValueError, match='for 3 rows'):
        distortion.DacStage([1.0, 2.0], 64, batch=3)
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.DacStage([1.0, 2.0], 64, offset=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match='no rows'):
        distortion.DacStage([], 64)
    with pytest.raises(ValueError, match='no rows'):
        distortion.DacStage(1.0, 64, batch=0)
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match='row 1: gain is not finite'):
            distortion.DacStage([1.0, bad], 64)
        with pytest.raises(ValueError, match='row 0: offset is not finite'):
            distortion.DacStage([1.0, 2.0], 64, offset=[bad, 0.0])
    for bits in (1, 0, 17, -3):
        with pytest.raises(ValueError, match='bits'):
            distortion.DacStage([1.0], 64, bits=bits)
    for bits, shift in ((16, 1), (14, 3), (12, -1), (2, 15)):
        with pytest.raises(ValueError, match='shift'):
            distortion.DacStage([1.0], 64, bits=bits, shift=shift)
    for k in (0, 3, 4, -1):
        with pytest.raises(ValueError, match='interleave'):
            distortion.DacStage([1.0] * 12, 64, interleave=k)
    with pytest.raises(ValueError, match='multiple'):
        distortion.DacStage([1.0, 2.0, 3.0], 64, interleave=2)
    with pytest.raises(ValueError, match='n >= 0'):
        distortion.DacStage([1.0], -1)
    with pytest.raises(ValueError, match='dtype'):
        distortion.DacStage([1.0], 64, dtype=np.int16)
    with pytest.raises(NotImplementedError):
        distortion.DacStage([1.0], 64, dtype=np.complex128)


def test_plan_refuses_before_any_device_work():
    for args in (([], [], 64), ([1.0, 2.0], [0.0], 64), ([1.0], [0.0], -1), ([np.nan], [0.0], 64),
                 ([1.0], [np.inf], 64), ([1.0], [0.0], 64, 1), ([1.0], [0.0], 64, 17), ([1.0], [0.0], 64, 14, 3),
                 ([1.0], [0.0], 64, 16, -1), ([1.0], [0.0], 64, 16, 0, 3), ([1.0], [0.0], 64, 16, 0, 2),
                 ([1.0], [0.0], 64, 16, 0, 1, np.int32)):
        with pytest.raises(ValueError):
            _engine.DacRowsPlan(*args)
    with pytest.raises(NotImplementedError):
        _engine.DacRowsPlan([1.0], [0.0], 64, dtype=np.complex64)


def test_wrapper_refuses_before_any_device_work():
    sig = np.zeros((2, 16))
    with pytest.raises(ValueError, match='2-D'):
        distortion.dac_codes_rows(np.zeros(16), 1.0)
    with pytest.raises(ValueError, match='2-D'):
        distortion.dac_codes_rows(np.zeros((2, 2, 4)), 1.0)
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.dac_codes_rows(sig, [1.0])
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.dac_codes_rows(sig, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.dac_codes_rows(sig, 1.0, offset=[0.0])
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match='not finite'):
            distortion.dac_codes_rows(sig, [1.0, bad])
        with pytest.raises(ValueError, match='not finite'):
            distortion.dac_codes_rows(sig, 1.0, offset=bad)
    with pytest.raises(ValueError, match='bits'):
        distortion.dac_codes_rows(sig, 1.0, bits=1)
    with pytest.raises(ValueError, match='shift'):
        distortion.dac_codes_rows(sig, 1.0, bits=14, shift=3)
    with pytest.raises(ValueError, match='interleave'):
        distortion.dac_codes_rows(sig, 1.0, interleave=3)
    with pytest.raises(ValueError, match='multiple'):
        distortion.dac_codes_rows(np.zeros((3, 16)), 1.0, interleave=2)
    with pytest.raises(ValueError):
        distortion.dac_codes_rows(np.zeros((0, 16)), 1.0)
    with pytest.raises(NotImplementedError):
        distortion.dac_codes_rows(sig + 0j, 1.0)
    codes, counts = distortion.dac_codes_rows(np.zeros((2, 0)), [1.0, 2.0], interleave=2, return_counts=True)
    assert codes.shape == (1, 0) and codes.dtype == np.int16                         # nothing to quantise
    assert counts.shape == (2, 3) and counts.dtype == np.int64 and not counts.any()
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.dac_codes_rows(np.zeros((2, 0)), [1.0])


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_dac_rows_plan_create', 'wfk_dac_rows_apply', 'wfk_dac_rows_plan_destroy',
                 'wfk_dac_rows_kernel_name'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_dac_rows_plan wfk_dac_rows_plan;' in src
    assert lib.wfk_abi_version() == 2


def test_library_refuses_before_any_device_work():
    """the C side's own refusals come before it looks for a device: WFK_EINVAL (-1) here, with the row named"""
    import ctypes as C
    lib = _engine.lib()
    g, o = (C.c_double * 2)(1.0, float('nan')), (C.c_double * 2)(0.0, 0.0)
    ok = (C.c_double * 2)(1.0, 2.0)
    h = C.c_void_p()
    create = lib.wfk_dac_rows_plan_create
    assert create(64, 2, 0, g, o, 16, 0, 1, C.byref(h)) == -1 and not h
    assert b'row 1: gain is not finite' in lib.wfk_last_error()
    for n, batch, kind, bits, shift, k in ((-1, 2, 0, 16, 0, 1), (64, 0, 0, 16, 0, 1), (64, 2, 2, 16, 0, 1),
                                           (64, 2, 0, 1, 0, 1), (64, 2, 0, 17, 0, 1), (64, 2, 0, 14, 3, 1),
                                           (64, 2, 0, 16, -1, 1), (64, 2, 0, 16, 0, 3), (64, 1, 0, 16, 0, 2),
                                           (2**62, 2, 0, 16, 0, 1), (2**62, 2, 0, 16, 0, 2)):
        assert create(n, batch, kind, ok, o, bits, shift, k, C.byref(h)) == -1 and not h, (n, batch, kind, bits, shift, k)
    assert lib.wfk_dac_rows_apply(None, None, 64, None, 64, None, None) == -1
    assert lib.wfk_dac_rows_plan_destroy(None) == 0
    assert lib.wfk_dac_rows_kernel_name(None, 0) == b''
