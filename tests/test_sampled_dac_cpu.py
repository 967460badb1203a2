"""The sampler that writes DAC codes itself (distortion.SampledDac, csrc/wfk_chain_dac.hip), without a device: every
refusal with its text, the symbols, and the tie condition the GPU referee test (tests/test_gpu_sampled_dac.py) rests
on, checked on the reference's own vectors (tests/golden/awg.npz)."""
import os
import re

import numpy as np
import pytest

import cases
import golden_io
import waveforms_amd as wf
from waveforms_amd import _engine, distortion, workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_CASES = sorted(n for n in cases.AWG_CASES if n != 'cplx_2g')
N = 2000
GRID = wl.awg_grid(N, 2e9)


def referee_parameters(y, bits=14):
    """the parameters of the golden cases: the row's peak at 1.25 of the top rail (rows clip), a fractional offset"""
    hi = 2**(bits - 1) - 1
    return 1.25 * hi / float(np.abs(y).max()), 3.25


def tie_zone(y, gain, offset):
    """samples whose exact x gain + offset lies within delta = gain * 1e-9 * max(1, max|y|) of a rounding tie: the
    sampler is held to 1e-9 * max(1, peak) of the golden vector, so only there may its code differ from the vector's"""
    delta = gain * 1e-9 * max(1.0, float(np.abs(y).max()))
    v = y * gain + offset
    return np.abs(v - np.floor(v) - 0.5) <= delta, delta


def chans(rows=2):
    return [wl.awg_channel(wf, c, N, 2e9) for c in range(rows)]


def test_refusals_come_before_any_device_work():
    for bits in (1, 0, 17, -3):
        with pytest.raises(ValueError, match=r'bits must lie in \[2, 16\]'):
            distortion.SampledDac(chans(), GRID, 1000.0, bits=bits)
    for bits, shift in ((16, 1), (14, 3), (12, -1), (2, 15)):
        with pytest.raises(ValueError, match=r'shift must lie in \[0, 16 - bits\]'):
            distortion.SampledDac(chans(), GRID, 1000.0, bits=bits, shift=shift)
    for k in (0, 3, 4, -1):
        with pytest.raises(ValueError, match='interleave must be 1 or 2'):
            distortion.SampledDac(chans(), GRID, 1000.0, interleave=k)
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match='row 1: gain is not finite'):
            distortion.SampledDac(chans(), GRID, [1.0, bad])
        with pytest.raises(ValueError, match='row 0: offset is not finite'):
            distortion.SampledDac(chans(), GRID, 1000.0, offset=[bad, 0.0])
    with pytest.raises(ValueError, match='3 rows are no multiple of the interleave 2'):
        distortion.SampledDac(chans(3), GRID, 1000.0, interleave=2)
    with pytest.raises(ValueError, match='3 rows are no multiple of the interleave 2'):
        distortion.SampledDac(chans(1), GRID, 1000.0, interleave=2, tile=3)
    with pytest.raises(ValueError, match='3 gain entries for 2 rows'):
        distortion.SampledDac(chans(), GRID, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match='1 offset entries for 2 rows'):
        distortion.SampledDac(chans(), GRID, 1000.0, offset=[0.0])
    with pytest.raises(ValueError, match='no rows'):
        distortion.SampledDac([], GRID, 1000.0)
    cplx = cases.AWG_CASES['cplx_2g'][0](wf, 2e9)
    with pytest.raises(NotImplementedError, match='complex rows'):
        distortion.SampledDac([cplx], GRID, 1000.0)
    with pytest.raises(NotImplementedError, match='complex rows'):
        distortion.SampledDac(chans(1) + [cplx], GRID, [1000.0, 2000.0])
    for fs in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='full scale'):
            distortion.SampledDac.from_full_scale(chans(), GRID, fs)
    with pytest.raises(ValueError, match='bits'):
        distortion.SampledDac.from_full_scale(chans(), GRID, 1.0, bits=17)


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_chain_dac_plan_create', 'wfk_chain_dac_plan_destroy', 'wfk_chain_dac_is_fused',
                 'wfk_chain_dac_unfused_reason', 'wfk_chain_dac_kernel_name', 'wfk_chain_dac_table_bytes',
                 'wfk_chain_dac_launch'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_chain_dac_plan wfk_chain_dac_plan;' in src
    assert hasattr(_engine, 'ChainDacPlan') and hasattr(distortion, 'SampledDac')
    assert lib.wfk_chain_dac_launch(None, None, 64, None, None, 0, None) == -1
    assert lib.wfk_chain_dac_plan_destroy(None) == 0
    assert lib.wfk_chain_dac_is_fused(None) == 0 and lib.wfk_chain_dac_kernel_name(None, 1) == b''


@pytest.mark.parametrize('name', REAL_CASES)
def test_referee_tie_zone_is_thin(name):
    """The GPU referee test compares codes exactly outside the tie zone.  That says something only if the zone is thin:
    at most 1e-3 of a case's samples may lie in it (measured: at most 2 samples per case)."""
    y = golden_io.npz('awg.npz')[name + '.y']
    assert not np.iscomplexobj(y)
    gain, offset = referee_parameters(y)
    zone, delta = tie_zone(y, gain, offset)
    print(f'{name}: {int(zone.sum())} of {len(y)} samples within {delta:.3g} LSB of a tie')
    assert delta < 0.01 and zone.sum() <= 1e-3 * len(y)
