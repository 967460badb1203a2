"""Per-row IIR stage, the parts that need no GPU: argument validation of `predistort_rows`, `distort_rows`
and `IirStage` (everything below fails before any device call), and the padding of a short row to the
common shape of a batch (`_engine.pack_sections_rows`), which must leave the row's filter unchanged."""
import numpy as np
import pytest
from scipy.signal import lfilter, lfiltic

from waveforms_amd import _engine, distortion


def _filters(taus, amps, rate=1e9):
    return [distortion.exp_decay_filter(a, t, rate) for a, t in zip(amps, taus)]


def test_names_exist():
    for name in ('IirStage', 'predistort_rows', 'distort_rows'):
        assert hasattr(distortion, name)
    assert hasattr(_engine, 'IirRowsPlan')


def test_predistort_rows_validation():
    sig = np.zeros((3, 100))
    f = _filters([100e-9], [0.02])
    with pytest.raises(ValueError):
        distortion.predistort_rows(np.zeros(100), [f])                    # 1-D signal
    with pytest.raises(ValueError):
        distortion.predistort_rows(sig, [f, f])                           # wrong number of rows
    with pytest.raises(ValueError):
        distortion.predistort_rows(sig, [f, f, f], initial=[0.1, 0.2])    # ragged initial
    with pytest.raises(ValueError):
        distortion.predistort_rows(sig, [f, f, f], zi=[np.zeros(1), np.zeros(2), np.zeros(1)])   # zi of the wrong shape
    with pytest.raises(ValueError):
        distortion.predistort_rows(sig, [f, f, f], zi=[np.zeros(1), np.zeros(1)])                # zi: wrong number of rows
    cf = [(np.array([1.0 + 1j, 0.5]), np.array([1.0, -0.9]))]
    with pytest.raises(NotImplementedError):
        distortion.predistort_rows(sig, [f, cf, f])                       # complex coefficients
    with pytest.raises(ValueError):
        distortion.distort_rows(sig, [[0.02, 100e-9]] * 2, 1e9)           # wrong number of rows


def test_iir_stage_validation():
    f = _filters([100e-9], [0.02])
    with pytest.raises(ValueError):
        distortion.IirStage([f, f], 100, 3)                               # two cascades for three rows
    with pytest.raises(ValueError):
        distortion.IirStage([f, f], 100, 2, dtype=np.int16)
    with pytest.raises(NotImplementedError):
        distortion.IirStage([f, [(np.array([1j, 0.5]), np.array([1.0, -0.9]))]], 100, 2)
    with pytest.raises(ValueError):
        distortion.IirStage([f, []], 100, 2)                              # a row without sections
    with pytest.raises(ValueError):
        distortion.IirStage(3.0, 100, 2)


def _dft2(b, a, x, zi):
    """direct form II transposed of ONE padded section (coefficient rows of equal length), as the kernel steps it"""
    m = len(b) - 1
    z = np.array(zi, dtype=np.float64)
    y = np.empty(len(x))
    for t, xx in enumerate(x):
        yy = b[0] * xx + z[0]
        for j in range(m - 1):
            z[j] = b[j + 1] * xx - a[j + 1] * yy + z[j + 1]
        z[m - 1] = b[m] * xx - a[m] * yy
        y[t] = yy
    return y, z


def test_padding_keeps_the_filter():
    rng = np.random.default_rng(5)
    rows = [[distortion.combine_filters(_filters(t, a))] for t, a in
            (([80e-9], [0.03]), ([50e-9, 900e-9, 3e-6], [0.02, -0.01, 0.015]), ([], []))]
    orders, bm, am, own = _engine.pack_sections_rows(rows)
    assert orders.tolist() == [3] and bm.shape == (3, 4) and am.shape == (3, 4)
    assert own == [[1], [3], [0]]
    x = rng.standard_normal(400)
    for r, row in enumerate(rows):
        b, a = row[0]
        b, a = np.atleast_1d(b), np.atleast_1d(a)
        zi = lfiltic(b, a, np.full(len(a) - 1, 0.2), np.full(len(b) - 1, 0.2))
        want, wzf = (lfilter(b, a, x, zi=zi) if len(zi) else (lfilter(b, a, x), np.zeros(0)))
        zpad = np.zeros(3)
        zpad[:len(zi)] = zi
        got, zf = _dft2(bm[r], am[r], x, zpad)
        m = max(len(a), len(b))
        if m > 1:        # the same recurrence on the row's own coefficients: padding changes nothing, bit for bit
            own_b, own_a = np.zeros(m), np.zeros(m)
            own_b[:len(b)], own_a[:len(a)] = b, a
            alone, zalone = _dft2(own_b, own_a, x, zi)
            assert np.array_equal(got, alone) and np.array_equal(zf[:m - 1], zalone)
        assert np.max(np.abs(got - want)) <= 1e-9 * max(1.0, np.abs(want).max())
        assert np.max(np.abs(zf[:len(wzf)] - wzf), initial=0.0) <= 1e-9
        assert not zf[len(wzf):].any()                                    # the padding entries stay zero


def test_padding_of_cascades_adds_pass_through_sections():
    f1, f2 = _filters([80e-9], [0.03])[0], _filters([400e-9], [-0.02])[0]
    orders, bm, am, own = _engine.pack_sections_rows([[f1], [f1, f2]])
    assert orders.tolist() == [1, 1] and own == [[1], [1, 1]]
    assert bm[0].tolist()[2:] == [1.0, 0.0] and am[0].tolist()[2:] == [1.0, 0.0]
    with pytest.raises(ValueError):
        _engine.pack_sections_rows([])
