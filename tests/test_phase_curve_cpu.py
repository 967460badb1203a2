"""Host side of `distortion.phase_curve` / `PhaseCurve` (no GPU): the referee the device tests use is the
reference's own function bit for bit, the probe plan's bracket table makes np.interp's choices, every case where
the reference raises is a ValueError before any device work, and the names are there."""
import importlib.util
import os

import numpy as np
import pytest

import phase_curve_ref as ref
from waveforms_amd import _engine, distortion

REFERENCE = '/root/reference/waveforms'


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='reference sources not on this machine')
@pytest.mark.parametrize('params,pw,start', ref.DEMO_CASES)
def test_restatement_is_the_reference_bit_for_bit(params, pw, start):
    """phase_curve_ref.restated (np.convolve + np.interp over lfilter on the combined (b, a)) against the live
    waveforms/distortion.py:349-366, loaded by file path (it needs NumPy / SciPy only)"""
    spec = importlib.util.spec_from_file_location('reference_distortion', os.path.join(REFERENCE, 'distortion.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for t in (ref.DEMO_T, np.float64(1e-7), np.array([-25e-6, 3e-7, 25e-6])):
        want = mod.phase_curve(t, params, ref.DF_DPHI, pw, start, ref.demo_wave_host, 2e9)
        got = ref.restated(t, params, ref.DF_DPHI, pw, start, ref.demo_wave_host, 2e9)
        assert type(got) is type(want) and np.shape(got) == np.shape(want)
        assert np.array_equal(got, want)


@pytest.mark.parametrize('params,pw,start', ref.DEMO_CASES[::3])
def test_longdouble_cascade_agrees_with_the_restatement_where_that_is_trustworthy(params, pw, start):
    """one and two time constants: the combined direct form in double is 1e-14 / 7e-12 of scale off the long-double
    curves, which agree with each other (cascade == combined filter in exact arithmetic)"""
    args = (ref.DEMO_T, params, ref.DF_DPHI, pw, start, ref.demo_wave_host, 2e9)
    want, casc, comb = ref.restated(*args), ref.longdouble_curve(*args), ref.combined_longdouble_curve(*args)
    s = ref.scale(want)
    print(f'{len(params) // 2} constants: restated vs combined ld {np.max(np.abs(want - comb)) / s:.3g}, '
          f'cascade ld vs combined ld {np.max(np.abs(casc - comb)) / s:.3g}')
    assert np.max(np.abs(want - comb)) < 1e-10 * s
    assert np.max(np.abs(casc - comb)) < 1e-10 * s


def test_bracket_table_makes_np_interp_s_choices():
    rng = np.random.default_rng(5)
    for tlist in (np.arange(80000) / 2e9 - 20e-6, np.sort(rng.uniform(-1, 1, 300)), np.array([0.0, 1.0])):
        n = len(tlist)
        span = tlist[-1] - tlist[0] + 1e-6
        t = np.concatenate([rng.uniform(tlist[0] - 0.2 * span, tlist[-1] + 0.2 * span, 2000),      # unsorted, clamped
                            tlist[rng.integers(0, n, 50)], tlist[[0, -1]],                         # exact grid points
                            [np.nan, -np.inf, np.inf, tlist[0] - 1.0, tlist[-1] + 1.0],
                            np.repeat(rng.uniform(tlist[0], tlist[-1], 5), 3),                     # repeated
                            np.nextafter(tlist[:3], np.inf), np.nextafter(tlist[-3:], -np.inf)])
        j, dx, w = _engine.probe_brackets(tlist, t)
        assert j.dtype == np.int64 and j.min() >= 0 and j.max() <= n - 1
        fp = rng.standard_normal(n)
        f0, f1 = fp[j], fp[np.minimum(j + 1, n - 1)]
        got = (f1 - f0) / w * dx + f0                      # the kernel's expression
        want = np.interp(t, tlist, fp)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 1
        ok = ~np.isnan(want)
        assert np.max(np.abs(got[ok] - want[ok])) <= 4 * np.finfo(float).eps * np.abs(fp).max()
        inside = ok & (t > tlist[0]) & (t < tlist[-1])
        assert np.all(tlist[j[inside]] <= t[inside]) and np.all(t[inside] < tlist[j[inside] + 1])
        assert np.all(dx[ok & ~inside] == 0) and np.all(j[ok & (t >= tlist[-1])] == n - 1)
        assert np.all(j[ok & (t <= tlist[0])] == 0)
        on = np.isin(t, tlist) & ok
        assert np.array_equal(got[on], want[on])           # a grid point gives the grid value itself
    with pytest.raises(_engine.EngineError):
        _engine.probe_brackets(np.array([0.0, 2.0, 1.0]), np.array([0.5]))
    with pytest.raises(_engine.EngineError):
        _engine.probe_brackets(np.array([0.0, np.nan]), np.array([0.5]))


def _no_wave(t):
    raise AssertionError('the wave must not be sampled before the arguments are checked')


@pytest.mark.parametrize('t,pw,start', [
    ([], 10e-9, 25e-9),                 # np.max of an empty t
    ([1e-6], 0.0, 0.5e-9),              # pulse points + start points == 0: np.convolve refuses an empty kernel
    ([1e-6], 10e-9, -20e-9),            # start points < 0: np.zeros of a negative length
    ([1e-6], -10e-9, 50e-9),            # pulse points < 0: np.ones of a negative length
    ([1e-6], 30e-6, 20e-6),             # a kernel longer than the signal: np.interp gets arrays of two lengths
    ([1e-6, np.nan], 10e-9, 25e-9),     # round(nan)
])
def test_value_errors_come_before_any_device_work(t, pw, start):
    with pytest.raises(ValueError):
        distortion.phase_curve(t, [-0.03, 0.1e-6], ref.DF_DPHI, pw, start, _no_wave, 2e9)
    with pytest.raises(ValueError):
        distortion.PhaseCurve(t, ref.DF_DPHI, pw, start, _no_wave, 2e9)
    with pytest.raises(ValueError):     # the referee raises in the same places
        ref.restated(np.asarray(t, dtype=float), [-0.03, 0.1e-6], ref.DF_DPHI, pw, start, ref.demo_wave_host, 2e9)


def test_names_are_exported():
    assert callable(distortion.phase_curve) and isinstance(distortion.PhaseCurve, type)
    for name in ('rows', 'rows_torch', 'jac', 'model', 'jac_model', 'step', 'close'):
        assert hasattr(distortion.PhaseCurve, name)
    assert hasattr(_engine, 'BoxProbePlan') and hasattr(_engine.IirRowsPlan, 'apply_shared_in')
    # curve_fit's default method is MINPACK's lmdif: h = sqrt(eps) * |p|, sqrt(eps) where p == 0
    h = distortion.PhaseCurve.step([-0.03, 0.0, 2.0])
    assert np.array_equal(h, np.sqrt(np.finfo(float).eps) * np.array([0.03, 1.0, 2.0]))
    assert np.array_equal(distortion.PhaseCurve.step([-0.5, 0.0], 1e-3), [0.5e-3, 1e-3])
