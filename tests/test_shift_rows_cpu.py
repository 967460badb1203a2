"""Per-row shift (distortion.ShiftStage / shift_rows), everything up to the point a device is needed: the referee
(tests/shift_rows_ref.py) against the live reference where its checkout is present, the (points, delta) split, the
argument checks that come before any device work, and the declarations of the header.

Bound of the referee against the reference: 4 * 2^-53 * B_i per element, B_i = |1 - d| |x[i - p]| + |d| |x[i - p - 1]|
(0 where y[i] is zero fill, and there the two agree exactly) -- derived, not measured: each side rounds two
products and one sum."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import shift_rows_ref as ref
from oracle import make_golden
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.isdir(os.path.join(make_golden.REF, 'waveforms'))

NS = (3, 4, 5, 17, 255, 256, 257, 4099)
DTS = (1.0, 0.5, 1 / 2e9)


def delays_of(n):
    return [0.0, 0.3, 1.0, 1.5, -0.25, -2.0, -3.7, 7.125, n - 0.5, -(n - 0.5), n + 2.0, -(n + 2.5)]


def grid():
    """(n, delay, dt): the listed delays as they stand and in units of dt (the same thing for dt = 1), so that the
    small steps see fractional delays too and not only rows pushed out altogether"""
    cases = []
    for n in NS:
        for dt in DTS:
            ds = delays_of(n)
            for d in ds + ([k * dt for k in ds] if dt != 1.0 else []):
                cases.append((n, d, dt))
        cases += [(n, 1.0, 0.1), (n, -0.3, 0.1)]      # 1.0 // 0.1 = 9: delta = 1 exactly
    return cases


def signal(n):
    return np.random.default_rng(1000 + n).normal(size=n) * np.exp(np.random.default_rng(n).uniform(-3, 3, n))


_REF_SCRIPT = r'''
import pickle, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle.make_golden import import_reference
import_reference()
from waveforms.distortion import shift
cases, signals = pickle.load(open(sys.argv[2], 'rb'))
pickle.dump([shift(signals[n], d, dt) for n, d, dt in cases], open(sys.argv[3], 'wb'))
'''


@pytest.fixture(scope='module')
def reference_results(tmp_path_factory):
    if not HAVE_REF:
        pytest.skip('reference sources not on this machine')
    d = tmp_path_factory.mktemp('ref_shift')
    script, cases, out = d / 'ref_shift.py', d / 'cases.pkl', d / 'out.pkl'
    script.write_text(_REF_SCRIPT)
    with open(cases, 'wb') as f:
        pickle.dump((grid(), {n: signal(n) for n in NS}), f)
    r = subprocess.run([sys.executable, str(script), ROOT, str(cases), str(out)], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out, 'rb') as f:
        return pickle.load(f)


def test_referee_matches_the_live_reference(reference_results):
    worst = 0.0
    cases = grid()
    assert len(cases) == len(reference_results)
    for (n, d, dt), want in zip(cases, reference_results):
        p, delta = ref.split(d, dt)
        assert 0.0 <= delta <= 1.0, (d, dt, p, delta)
        y, B = ref.shift_ref(signal(n), p, delta)
        assert want.shape == y.shape
        diff = np.abs(y - want)
        assert np.all(diff[B == 0] == 0.0), (n, d, dt)
        assert np.all(diff <= ref.BOUND * B), (n, d, dt, float(np.max(diff / np.maximum(B, 1e-300))) / 2.0**-53)
        worst = max(worst, float(np.max(diff[B > 0] / B[B > 0], initial=0.0)) / 2.0**-53)
    print(f'{len(cases)} cases: worst |diff| = {worst:.3g} * 2^-53 * B')


def test_split_follows_python_floor_division():
    assert ref.split(1.0, 0.1) == (9, 1.0)                       # not floor(1.0 / 0.1) = 10
    assert distortion._shift_split('t', [1.0, 0.3, -0.25, 7.125, -3.7], 1.0)[0] == [1, 0, -1, 7, -4]
    for d, dt in ((1.0, 0.1), (0.7, 0.1), (-0.3, 0.1), (1.5, 0.5), (-3.7, 1.0), (7.125 / 2e9, 1 / 2e9), (0.0, 1.0)):
        (p,), (delta,) = distortion._shift_split('t', [d], dt)
        assert (p, delta) == ref.split(d, dt) and 0.0 <= delta <= 1.0
    assert distortion._shift_split('t', [1.0], 0.1) == ([9], [1.0])
    # delta = 1 is the shift by one more whole sample, up to the rounding of 0 * x + 1 * x[j - 1]
    x = signal(17)
    y1, _ = ref.shift_ref(x, 9, 1.0)
    y0, _ = ref.shift_ref(x, 10, 0.0)
    assert np.array_equal(y1, y0)


def test_referee_properties():
    x = signal(257)
    for p in (-300, -257, 257, 300):
        y, B = ref.shift_ref(x, p, 0.25)
        assert not y.any() and not B.any()
    y, _ = ref.shift_ref(x, 3, 0.0)
    assert np.array_equal(y[3:], x[:-3]) and not y[:3].any()
    y, _ = ref.shift_ref(x, -2, 0.5)
    assert y[-1] == 0.0 and y[-2] == 0.0 and y[-3] == 0.5 * x[-1] + 0.5 * x[-2]      # nothing from past the end
    y, _ = ref.shift_ref(x, 0, 0.25)
    assert y[0] == 0.75 * x[0]
    for n in (1, 2):                                                                  # rows keep n
        assert ref.shift_ref(x[:n], 0, 0.5)[0].shape == (n,)


def test_wrappers_refuse_before_any_device_work():
    sig = np.zeros((2, 16))
    with pytest.raises(ValueError, match='2-D'):
        distortion.shift_rows(np.zeros(16), 1e-9, 1e-9)
    with pytest.raises(ValueError, match='2-D'):
        distortion.shift_rows(np.zeros((2, 2, 4)), 1e-9, 1e-9)
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.shift_rows(sig, [1e-9], 1e-9)
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.shift_rows(sig, [1e-9, 2e-9, 3e-9], 1e-9)
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match='not finite'):
            distortion.shift_rows(sig, [1e-9, bad], 1e-9)
    for dt in (0.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='dt'):
            distortion.shift_rows(sig, 1e-9, dt)
    with pytest.raises(NotImplementedError):
        distortion.shift_rows(sig + 0j, 1e-9, 1e-9)
    out = distortion.shift_rows(np.zeros((2, 0)), [1e-9, -2e-9], 1e-9)                # nothing to move
    assert out.shape == (2, 0)
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.shift_rows(np.zeros((2, 0)), [1e-9], 1e-9)


def test_stage_refuses_before_any_device_work():
    with pytest.raises(ValueError, match='batch'):
        distortion.ShiftStage(1e-9, 64, 1e-9)                                         # a scalar needs batch=
    with pytest.raises(ValueError, match='for 3 rows'):
        distortion.ShiftStage([1e-9, 2e-9], 64, 1e-9, batch=3)
    with pytest.raises(ValueError, match='no rows'):
        distortion.ShiftStage([], 64, 1e-9)
    with pytest.raises(ValueError):
        distortion.ShiftStage(1e-9, 64, 1e-9, batch=0)
    with pytest.raises(ValueError, match='not finite'):
        distortion.ShiftStage([0.0, np.nan], 64, 1e-9)
    with pytest.raises(ValueError, match='dt'):
        distortion.ShiftStage([0.0], 64, 0.0)
    with pytest.raises(ValueError, match='n >= 0'):
        distortion.ShiftStage([0.0], -1, 1e-9)
    with pytest.raises(ValueError, match='dtype'):
        distortion.ShiftStage([0.0], 64, 1e-9, dtype=np.int16)
    with pytest.raises(NotImplementedError):
        distortion.ShiftStage([0.0], 64, 1e-9, dtype=np.complex128)
    for points, deltas in (([0], [1.5]), ([0], [-0.25]), ([0], [np.nan]), ([0, 1], [0.5]), ([], [])):
        with pytest.raises(ValueError):
            _engine.ShiftRowsPlan(points, deltas, 64)


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_shift_rows_plan_create', 'wfk_shift_rows_apply', 'wfk_shift_rows_plan_destroy',
                 'wfk_shift_rows_kernel_name'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_shift_rows_plan wfk_shift_rows_plan;' in src
    assert lib.wfk_abi_version() == 2
