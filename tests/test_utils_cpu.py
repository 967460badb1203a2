"""waveforms_amd.utils without a GPU: getFTMatrix against its closed form and (where the reference checkout is
present) against the reference's own getFTMatrix bit for bit, freeze / shift against the reference's behaviour,
and the Demodulator's argument checks that come before any device work."""
import os
import pickle
import subprocess
import sys
from types import MappingProxyType

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import make_golden
from waveforms_amd import utils
from waveforms_amd.utils import Demodulator, freeze, getFTMatrix, shift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.isdir(os.path.join(make_golden.REF, 'waveforms'))

_rng = np.random.default_rng(11)
_W1 = _rng.uniform(0.5, 1.5, 64)
_W2 = _rng.uniform(-1, 1, (3, 64))
_WC = _rng.normal(size=64) + 1j * _rng.normal(size=64)

# (fList, numOfPoints, phaseList, weight, sampleRate)
CASES = {
    'two_tones': ([-12.7e6, 32.8e6], 1000, None, None, 1e9),
    'phases': ([10e6, 20e6, 30e6], 256, [0.1, -0.7, 2.0], None, 2e9),
    'weight_1d': ([5e6, 50e6], 64, None, _W1, 1e9),
    'weight_2d': ([5e6, 50e6, 75e6], 64, [0.0, 0.5, 1.0], _W2, 1e9),
    'weight_complex': ([5e6, -5e6], 64, None, _WC, 1e9),
    'empty_weight_phase': ([1e6, 2e6], 128, [], np.zeros(0), 1e9),
    'short_phase_list': ([1e6, 2e6, 3e6, 4e6], 100, [0.3, 0.4], None, 1e9),
    'fewer_weight_rows': ([1e6, 2e6, 3e6, 4e6], 64, None, _W2[:2], 1e9),
    'int_flist': ([3, 7, 11], 50, None, None, 100),
    'n1': ([1e6], 1, None, None, 1e9),
    'n100k': ([-1.5e6, 40e6, 123.456e6], 100000, [0.25, 0.5, 0.75], None, 1e9),
    'fft_bins': (np.fft.fftfreq(16), 16, None, None, 1),
}


def closed_form(fList, N, phaseList, weight, sr):
    t = np.linspace(0, N / sr, N, endpoint=False)
    if weight is None or len(weight) == 0:
        weight = np.full(N, 2 / N)
    weight = np.asarray(weight)
    rows = [weight] * len(fList) if weight.ndim == 1 else list(weight)
    phases = np.zeros(len(fList)) if phaseList is None or len(phaseList) == 0 else list(phaseList)
    nf = min(len(fList), len(phases), len(rows))
    cols = [rows[j] * np.exp(-1j * (2 * np.pi * fList[j] * t + phases[j])) for j in range(nf)]
    return np.stack(cols, axis=1)


@pytest.mark.parametrize('name', sorted(CASES))
def test_getFTMatrix_closed_form(name):
    args = CASES[name]
    e = getFTMatrix(*args)
    want = closed_form(*args)
    assert e.dtype == np.complex128 and e.shape == want.shape
    assert np.array_equal(e, want)


def test_getFTMatrix_truncates_like_zip():
    assert getFTMatrix(*CASES['short_phase_list']).shape == (100, 2)
    assert getFTMatrix(*CASES['fewer_weight_rows']).shape == (64, 2)
    assert getFTMatrix([1e6, 2e6], 10, weight=np.ones((5, 10))).shape == (10, 2)


def test_getFTMatrix_fft_identity():
    rng = np.random.default_rng(3)
    for N in (16, 1000, 1001):
        x = rng.normal(size=(4, N))
        e = getFTMatrix(np.fft.fftfreq(N), N, sampleRate=1)
        assert np.allclose(2 * np.fft.fft(x, axis=-1) / N, x @ e)


def test_getFTMatrix_docstring_example():
    N, sr, f1, f2 = 1000, 1e9, -12.7e6, 32.8e6
    t = np.arange(N) / sr
    sig = 0.8 * np.sin(2 * np.pi * f1 * t) + 0.2 * np.cos(2 * np.pi * f2 * t)
    got = sig @ getFTMatrix([f1, f2], N, sampleRate=sr)
    assert np.allclose(got, [-0.00766509 - 0.79518987j, 0.19531432 + 0.00207068j], atol=1e-8)


_REF_SCRIPT = r'''
import pickle, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle.make_golden import import_reference
import_reference()
from waveforms import utils as U
cases = pickle.load(open(sys.argv[2], 'rb'))
res = {name: U.getFTMatrix(*args) for name, args in cases.items()}
import scipy.sparse as sp
arr = np.arange(4.0)
f = U.freeze({'a': [1, 2, (3, [4])], 'b': {7, 8}, 'c': bytearray(b'ab'), 'd': arr, 'e': None, 'g': 2.5})
res['freeze'] = (type(f).__name__, f['a'], type(f['b']).__name__, sorted(f['b']), f['c'], f['d'].flags.writeable,
                 f['e'], f['g'])
mats = {fmt: sp.random(5, 5, density=0.4, format=fmt, random_state=1) for fmt in ('csr', 'csc', 'bsr', 'coo')}
for fmt, m in mats.items():
    U.freeze(m)
    fl = [m.data.flags.writeable]
    fl += [m.indices.flags.writeable, m.indptr.flags.writeable] if fmt != 'coo' else [m.row.flags.writeable,
                                                                                       m.col.flags.writeable]
    res['sparse_' + fmt] = fl
sig = np.random.default_rng(5).normal(size=200)
res['shift'] = [U.shift(sig, d, 0.5) for d in (0.0, 1.5, -2.0, 8.5)]
pickle.dump(res, open(sys.argv[3], 'wb'))
'''


@pytest.fixture(scope='module')
def reference_results(tmp_path_factory):
    if not HAVE_REF:
        pytest.skip('reference sources not on this machine')
    d = tmp_path_factory.mktemp('ref_utils')
    script, cases, out = d / 'ref_utils.py', d / 'cases.pkl', d / 'out.pkl'
    script.write_text(_REF_SCRIPT)
    with open(cases, 'wb') as f:
        pickle.dump(CASES, f)
    r = subprocess.run([sys.executable, str(script), ROOT, str(cases), str(out)], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out, 'rb') as f:
        return pickle.load(f)


@pytest.mark.parametrize('name', sorted(CASES))
def test_getFTMatrix_matches_reference_bitwise(reference_results, name):
    want = reference_results[name]
    got = getFTMatrix(*CASES[name])
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want)


def test_freeze_matches_reference(reference_results):
    arr = np.arange(4.0)
    f = freeze({'a': [1, 2, (3, [4])], 'b': {7, 8}, 'c': bytearray(b'ab'), 'd': arr, 'e': None, 'g': 2.5})
    got = (type(f).__name__, f['a'], type(f['b']).__name__, sorted(f['b']), f['c'], f['d'].flags.writeable,
           f['e'], f['g'])
    assert got == reference_results['freeze']
    for fmt in ('csr', 'csc', 'bsr', 'coo'):
        m = sp.random(5, 5, density=0.4, format=fmt, random_state=1)
        freeze(m)
        fl = [m.data.flags.writeable]
        fl += [m.indices.flags.writeable, m.indptr.flags.writeable] if fmt != 'coo' else [m.row.flags.writeable,
                                                                                           m.col.flags.writeable]
        assert fl == reference_results['sparse_' + fmt], fmt


def test_shift_matches_reference_for_whole_sample_delays(reference_results):
    # whole-sample delays stay on the host (no fractional tap); fractional ones run the device FIR
    sig = np.random.default_rng(5).normal(size=200)
    for k, d in enumerate((0.0, 1.5, -2.0, 8.5)):
        assert np.array_equal(shift(sig, d, 0.5), reference_results['shift'][k])


def test_freeze_behaviour():
    f = freeze({'a': [1, [2]], 's': {1}, 'b': bytearray(b'q')})
    assert isinstance(f, MappingProxyType) and f['a'] == (1, (2,)) and f['s'] == frozenset({1}) and f['b'] == b'q'
    a = np.zeros(3)
    assert freeze(a) is a and not a.flags.writeable
    m = sp.csr_matrix(np.eye(3))
    freeze(m)
    assert not (m.data.flags.writeable or m.indices.flags.writeable or m.indptr.flags.writeable)
    assert freeze(3) == 3 and freeze('s') == 's' and freeze(None) is None


def test_shift_is_the_distortion_shift():
    from waveforms_amd import distortion
    assert utils.shift is distortion.shift
    sig = np.arange(10.0)
    assert np.array_equal(shift(sig, 2.0, 1.0), np.r_[0, 0, sig[:-2]])
    assert np.array_equal(shift(sig, -3.0, 1.0), np.r_[sig[3:], 0, 0, 0])


def test_demodulator_rejects_bad_arguments_before_the_device():
    with pytest.raises(ValueError):
        Demodulator([1e6], 100, dtype=np.int32)
    with pytest.raises(ValueError):
        Demodulator([1e6], 100, dtype=np.complex128)
    with pytest.raises(ValueError):
        Demodulator.from_matrix(np.ones(10, complex))
    with pytest.raises(ValueError):
        Demodulator.from_matrix(np.ones((0, 3), complex))
    with pytest.raises(ValueError):
        Demodulator.from_matrix(np.ones((10, 0), complex))
    with pytest.raises(ValueError):     # no tones: getFTMatrix returns an empty 1-D array
        Demodulator([], 10)
