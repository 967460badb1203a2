"""The round-once bound of float rows (tests/float_rows_ref.py) has teeth -- shown without a device, on the exact inputs
and cascades tests/test_gpu_float_rows.py runs on one:

  * the float64 referee rounded once passes `check` and `check_exactly_rounded`;
  * the recurrence with float32 COEFFICIENTS, and the recurrence IN float32, miss the bound by at least 100 x on every
    cascade (measured here with NumPy / SciPy: 8.3e3 at the least on the shared cascades, 2.9e3 on the per-row ones, 170
    on the chain's; the 100 keeps the device test from being vacuous, it is not a device measurement);
  * one rounding PER SECTION misses it on every cascade of three first-order sections (measured: 2.0 .. 19);
  * the same wrong forms PASS cases.FP32_TOL of the peak on the Butterworth cascades, and the wrong FIR forms pass the FIR
    tests' 1e-5: that is the gap the device tests close, on record here.

What is measured is printed (`pytest -s`)."""
import functools

import numpy as np
import pytest

import float_rows_ref as fr
from cases import FP32_TOL, FP64_FIR_TOL, FP64_IIR_TOL

MISS = 100.0            # the floor for the float32-coefficient and float32-recurrence forms
BUTTERWORTH = ('three_launch', 'single_pass', 'persistent')


def _forms(what, secs, x32, zi, initial, tol64):
    """referee rounded once passes; -> {wrong form: (worst ratio, index, share over, worst / peak)}"""
    want, _ = fr.iir_reference(secs, x32.astype(np.float64), zi, initial)
    fr.check(want.astype(np.float32), want, tol64, f'{what} rounded once')
    fr.check_exactly_rounded(want.astype(np.float32), want, tol64, f'{what} rounded once')
    bound = fr.round_once_bound(want, tol64)
    out = {}
    for name, got in fr.wrong_forms(secs, x32, zi, initial).items():
        assert got.dtype == np.float32 and got.shape == want.shape
        out[name] = fr.report(got, want, bound)
        print(f'{what} {name}: worst |diff| / bound = {out[name][0]:.3g}, {100 * out[name][2]:.3g} % over, '
              f'worst |diff| / peak = {out[name][3]:.3g} (old bound {FP32_TOL:g})')
    return want, out


@functools.lru_cache(maxsize=None)
def _shared(case):
    secs, rows, n, _, _, _, tol64 = fr.SHARED_CASES[case]
    x32 = fr.shared_input(rows, n)
    zi = fr.state_input(rows, sum(fr.orders_of(secs)))
    return (secs, x32, zi, tol64) + _forms(case, secs, x32, zi, fr.INITIAL, tol64)


@pytest.mark.parametrize('case', sorted(set(fr.SHARED_CASES) - {'gain'}))
def test_shared_cascades_wrong_forms_miss(case):
    _, _, _, _, _, forms = _shared(case)
    assert forms['f32_coefficients'][0] >= MISS and forms['f32_recurrence'][0] >= MISS, forms
    if case in BUTTERWORTH:
        # two biquads / one: what the suite looked at before -- the wrong forms are 10 x and more inside it
        assert all(f[3] <= FP32_TOL / 10 for f in forms.values()), forms
        assert forms['round_per_section'][0] > 1.0 or len(fr.SHARED_CASES[case][0]) == 1, forms


def test_gain_has_no_wrong_form():
    """0.5 / 2.0 is a float32 value and the product of a float by 0.25 is exact: every form IS the rounded referee but
    for `initial`, which the float32 recurrence subtracts and adds with a rounding each (that alone is over the bound)"""
    secs, x32, _, tol64, want, forms = _shared('gain')
    assert tol64 == fr.TOL64_GAIN
    assert np.array_equal(fr.wrong_forms(secs, x32, None, fr.INITIAL)['f32_coefficients'], want.astype(np.float32))
    assert forms['f32_recurrence'][0] > 1.0


@pytest.mark.parametrize('case', ['order3', 'order6'])
def test_single_sections_of_order_3_and_6_have_a_referee(case):
    """scipy's double lfilter on these direct forms is itself within a tenth of the bound of the long-double recurrence"""
    secs, x32, zi, tol64, _, _ = _shared(case)
    err = fr.referee_self_error(secs, x32, zi, fr.INITIAL)
    print(f'{case}: scipy against the long-double recurrence {err:.3g} of the scale (tol64 {tol64:g})')
    assert err <= 0.1 * tol64


@pytest.mark.parametrize('nsec,order', fr.ROW_SHAPES)
def test_per_row_cascades_wrong_forms_miss(nsec, order):
    x32 = fr.shared_input(3, fr.N_ROWS)
    zi = fr.state_input(3, nsec * order)
    for r, secs in enumerate(fr.row_cascades(nsec, order)):
        what = f'rows<{nsec},{order}> row {r}'
        ini = float(fr.ROW_INITIAL[r])
        _, forms = _forms(what, secs, x32[r:r + 1], zi[r:r + 1], ini, fr.TOL64_ROWS)
        assert forms['f32_coefficients'][0] >= MISS and forms['f32_recurrence'][0] >= MISS, (what, forms)
        if (nsec, order) == (3, 1):
            assert forms['round_per_section'][0] > 1.0, (what, forms)
        if order >= 3:
            err = fr.referee_self_error(secs, x32[r:r + 1], zi[r:r + 1], ini)
            print(f'{what}: scipy against the long-double recurrence {err:.3g} of the scale')
            assert err <= 0.1 * fr.TOL64_ROWS


def test_chain_cascades_wrong_forms_miss():
    x32 = fr.shared_input(3, fr.N_AWG)
    for r, secs in enumerate(fr.chain_cascades()):
        _, forms = _forms(f'chain row {r}', secs, x32[r:r + 1], None, float(fr.CHAIN_INITIAL[r]), FP64_IIR_TOL)
        assert forms['f32_coefficients'][0] >= MISS and forms['f32_recurrence'][0] >= MISS, (r, forms)


def test_exactly_rounded_rejects_one_rounding_per_section():
    secs = fr.row_cascades(3, 1)[0]
    x32 = fr.shared_input(3, fr.N_ROWS)[:1]
    want, _ = fr.iir_reference(secs, x32.astype(np.float64), None, 0.25)
    with pytest.raises(AssertionError, match='not float32'):
        fr.check_exactly_rounded(fr.wrong_forms(secs, x32, None, 0.25)['round_per_section'], want, fr.TOL64_ROWS, 'wrong')
    with pytest.raises(AssertionError, match='over the bound'):
        fr.check(fr.wrong_forms(secs, x32, None, 0.25)['round_per_section'], want, fr.TOL64_ROWS, 'wrong')


def test_chain_allowance_covers_a_rounded_input_and_little_else():
    """float32(F64(float32(s64))) is inside round_once_bound + the allowance, which stays a small multiple of one
    float rounding of the peak (it is a BOUND on the input rounding carried through |h|, not slack)"""
    x = fr.shared_input(3, fr.N_AWG).astype(np.float64) * (1 + 2.0**-30)        # a double row that float32 rounds
    for r, secs in enumerate(fr.chain_cascades()):
        ini = float(fr.CHAIN_INITIAL[r])
        want, _ = fr.iir_reference(secs, x[r:r + 1], None, ini)
        got, _ = fr.iir_reference(secs, x[r:r + 1].astype(np.float32).astype(np.float64), None, ini)
        extra = fr.chain_input_allowance(secs, x[r], 1e-9)
        fr.check(got.astype(np.float32), want, FP64_IIR_TOL, f'chain row {r} from a rounded input', extra[None, :])
        gain = np.abs(fr.impulse_response(secs, fr.N_AWG)).sum()
        assert extra.max() <= 1.01 * gain * (fr.EPS32 * np.abs(x[r]).max() + 1e-9 * fr.scale(x[r]))


@pytest.mark.parametrize('K', [1024, 2401, 64])
def test_fir_wrong_forms_miss(K):
    """The FIR is class B on the device (float transforms); the ROUND-ONCE bound against the double convolution is what
    its float rows do NOT meet, by three orders of magnitude, while the FIR tests' 1e-5 of the peak accepts them by as
    much.  Narrowed taps miss by less (12 .. 82: their errors average over K random taps) -- over the bound, printed."""
    x32 = fr.shared_input(4, 20011)
    ker = fr.fir_kernel(K, K)
    want = fr.fir_reference(x32, ker)
    fr.check(want.astype(np.float32), want, FP64_FIR_TOL, f'FIR K={K} rounded once')
    bound = fr.round_once_bound(want, FP64_FIR_TOL)
    forms = {k: fr.report(v, want, bound) for k, v in fr.fir_wrong_forms(x32, ker).items()}
    for k, f in forms.items():
        print(f'FIR K={K} {k}: worst |diff| / bound = {f[0]:.3g}, {100 * f[2]:.3g} % over, worst |diff| / peak = {f[3]:.3g}')
    assert forms['f32_transform'][0] >= MISS and forms['f32_taps'][0] > 1.0, forms
    assert all(f[3] <= 1e-5 / 10 for f in forms.values()), forms
