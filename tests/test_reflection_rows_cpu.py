"""Per-row reflection / delay stage, everything up to the point a device is needed: argument handling of
distortion.ReflectionStage and the three NumPy wrappers, the host term packer, the quad-precision phase step, the
library's symbols and the header as plain C."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wrapper_terms_broadcast_and_ragged_rows():
    terms = distortion._reflection_rows_terms('reflection_rows', 'reflect', 3, 0.1, [1e-9, 2e-9, 3e-9])
    assert terms == [[('reflect', 0.1, 1e-9)], [('reflect', 0.1, 2e-9)], [('reflect', 0.1, 3e-9)]]
    terms = distortion._reflection_rows_terms('reflection_rows', 'correct', 2, [0.1, -0.2], 5e-9)
    assert terms == [[('correct', 0.1, 5e-9)], [('correct', -0.2, 5e-9)]]
    # a row may give sequences: several reflections; a scalar goes with every entry of the other's sequence
    terms = distortion._reflection_rows_terms('reflection_rows', 'reflect', 3, [0.1, [0.2, 0.05], [0.3, 0.1]],
                                              [1e-9, [2e-9, 4e-9], 7e-9])
    assert terms == [[('reflect', 0.1, 1e-9)], [('reflect', 0.2, 2e-9), ('reflect', 0.05, 4e-9)],
                     [('reflect', 0.3, 7e-9), ('reflect', 0.1, 7e-9)]]
    assert distortion._reflection_rows_terms('reflection_rows', 'reflect', 2, [[], 0.1], [[], 1e-9])[0] == []
    assert distortion._delay_rows_terms(2, -3e-9) == [[('delay', -3e-9)]] * 2
    assert distortion._delay_rows_terms(2, [1e-9, 0.0]) == [[('delay', 1e-9)], [('delay', 0.0)]]
    with pytest.raises(ValueError, match='2 A entries for 3 rows'):
        distortion._reflection_rows_terms('reflection_rows', 'reflect', 3, [0.1, 0.2], 1e-9)
    with pytest.raises(ValueError, match='row 1 has 2 amplitudes and 3 delays'):
        distortion._reflection_rows_terms('reflection_rows', 'reflect', 2, [0.1, [0.1, 0.2]], [1e-9, [1e-9, 2e-9, 3e-9]])
    with pytest.raises(ValueError):
        distortion._delay_rows_terms(3, [1e-9, 2e-9])


def test_wrappers_refuse_before_any_device_work():
    sig = np.zeros((2, 16))
    for fn in (distortion.reflection_rows, distortion.correct_reflection_rows):
        with pytest.raises(ValueError, match='2-D'):
            fn(np.zeros(16), 0.1, 1e-9, 1e9)
        with pytest.raises(ValueError, match='for 2 rows'):
            fn(sig, [0.1, 0.2, 0.3], 1e-9, 1e9)
        with pytest.raises(ValueError, match=r'\|A\| < 1'):
            fn(sig, [0.1, 1.0], 1e-9, 1e9)
        with pytest.raises(ValueError, match='at most'):
            fn(sig, [[0.01] * (_engine.SPEC_ROWS_MAX_TERMS + 1), 0.1], 1e-9, 1e9)
        with pytest.raises(NotImplementedError):
            fn(sig + 0j, 0.1, 1e-9, 1e9)
    with pytest.raises(ValueError, match='2-D'):
        distortion.delay_rows(np.zeros(16), 1e-9, 1e9)
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.delay_rows(sig, [1e-9], 1e9)
    with pytest.raises(ValueError, match='not finite'):
        distortion.delay_rows(sig, [1e-9, np.inf], 1e9)
    assert distortion.delay_rows(np.zeros((2, 0)), 1e-9, 1e9).shape == (2, 0)      # nothing to transform


def test_term_packer_and_stage_arguments():
    terms, counts = _engine.pack_spec_terms([[('reflect', 0.1, 1e-9), ('delay', -2e-9)], [], [('correct', -0.3, 5e-9)]])
    assert terms.dtype.itemsize == 24 and list(counts) == [2, 0, 1] and counts.dtype == np.int32
    assert [tuple(t) for t in terms] == [(0, 0, 0.1, 1e-9), (2, 0, 0.0, -2e-9), (1, 0, -0.3, 5e-9)]
    full = [('delay', 1e-9)] * _engine.SPEC_ROWS_MAX_TERMS
    assert list(_engine.pack_spec_terms([full])[1]) == [_engine.SPEC_ROWS_MAX_TERMS]
    bad = [[[('echo', 0.1, 1e-9)]], [[('reflect', 0.1)]], [[('delay', 0.1, 1e-9)]], [[(0, 0.1, 1e-9)]], [[()]],
           [full + [('delay', 1e-9)]], [[('reflect', 1.0, 1e-9)]], [[('correct', -1.5, 1e-9)]],
           [[('reflect', np.nan, 1e-9)]], [[('delay', np.nan)]], []]
    for rows in bad:
        with pytest.raises(ValueError):
            _engine.pack_spec_terms(rows)
        with pytest.raises(ValueError):                     # the stage refuses them before it asks for a device
            distortion.ReflectionStage(rows, 64, 1e9)
    for n, fs, dtype in ((0, 1e9, np.float64), (64, 0.0, np.float64), (64, np.nan, np.float64), (64, 1e9, np.int16)):
        with pytest.raises(ValueError):
            distortion.ReflectionStage([[('delay', 1e-9)]], n, fs, dtype)


def test_header_constants_match():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    assert int(re.search(r'#define WFK_SPEC_ROWS_MAX_TERMS (\d+)', src).group(1)) == _engine.SPEC_ROWS_MAX_TERMS
    m = re.search(r'enum \{ WFK_SPEC_REFLECT = (\d), WFK_SPEC_CORRECT = (\d), WFK_SPEC_DELAY = (\d) \}', src)
    assert [int(g) for g in m.groups()] == [_engine.SPEC_KINDS[k] for k in ('reflect', 'correct', 'delay')]


def test_phase_step_is_a_double_double_of_the_exact_quotient():
    """c = tau fs / n as (hi, lo): below 1e-30 relative of the exact rational value of the doubles' quotient"""
    rng = np.random.default_rng(3)
    cases = [(5e-6, 2e9, 65536), (12.5e-9, 1e9, 10007), (-31e-9, 2e9, 30000), (200e-9, 2e9, 1), (1e-9 / 3, 2.4e9, 10**7)]
    cases += [(float(rng.uniform(-1e-5, 1e-5)), float(10**rng.uniform(6, 10)), int(rng.integers(1, 10**7)))
              for _ in range(20)]
    for tau, fs, n in cases:
        hi, lo = _engine.spec_phase_step(tau, fs, n)
        exact = Fraction(tau) * Fraction(fs) / n
        assert hi == float(exact)
        assert abs(Fraction(hi) + Fraction(lo) - exact) <= abs(exact) * Fraction(1, 10**30), (tau, fs, n)
    assert _engine.spec_phase_step(0.0, 1e9, 5) == (0.0, 0.0)


def test_symbols_and_plain_c_consumer(tmp_path):
    lib = _engine.lib()
    for name in ('wfk_spectral_rows_plan_create', 'wfk_spectral_rows_apply', 'wfk_spectral_rows_plan_destroy',
                 'wfk_spectral_rows_phase_step'):
        assert hasattr(lib, name), name
    exe = tmp_path / 'spectral_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'spectral_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = ''
    try:   # same runtime-loading order as _engine.lib(): torch's bundled HIP runtime first
        import torch
        torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    except Exception:
        pass
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'spectral_rows_smoke ok' in r.stdout
