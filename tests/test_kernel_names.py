"""What `kernel_name()` answers for every shape of sampler launch, on the CPU (plans compile and name themselves without
a device), against names recorded before the launch decision was given one owner (tests/golden/kernel_names.json:
`python oracle/make_golden.py names` rewrites it from the library in the tree).  About a hundred assertions in this suite
and every tool read the name to learn which tier ran: it must stay byte for byte what it was."""
import json
import os

import numpy as np
import pytest

import cases
import waveforms_amd as wf
from waveforms_amd import _engine, _flatten, workloads as wl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kernel_names.json')
DTYPES = (np.float64, np.float32, np.complex128, np.complex64)
AWG = wl.awg_grid(20000, 2e9)
W = wl.SPAN


def _awg(extra=None):
    w = wl.awg_channel(wf, 0, 20000, 2e9)
    return [w if extra is None else w + extra]


def _pulse_train(mk, n, period, t0=0.0, seed=13):
    rng = np.random.default_rng(seed)
    return wl._tree_sum([rng.uniform(0.3, 1) * mk(k, rng) >> (t0 + (k + 0.5) * period) for k in range(n)])


def _hann(m=1000, a=1.0):
    return wf.samplingPoints(-W / 2, W / 2, np.hanning(m) * a)


def _corr_short():     # fast carriers far from t = 0 at an AWG rate: family 6 of the short tier
    rng = np.random.default_rng(3)
    t0, w = 1e-3, wf.zero()
    for k in range(100):
        I, Q = wf.mixing(wf.gaussian(20e-9), freq=rng.uniform(-3e8, 3e8), phase=rng.uniform(0, 6), DRAGScaling=1e-10)
        w = w + ((rng.uniform(0.2, 1) * (I if k % 2 else Q)) >> (t0 + (k + 0.5) * 30e-9))
    return [w], ('arange', t0, t0 + 8000 / 2e9, 1 / 2e9)


def _far(t_center=16e-3, f=300e6, edge=False):     # the same on a fine grid: the corrected lean build
    I, Q = wf.mixing(0.7 * wf.gaussian(40e-9) >> t_center, freq=f, phase=1.0, DRAGScaling=1e-10)
    chans = [(wf.square(1e-6, edge=200e-9) >> t_center) * wf.cos(2 * np.pi * f)] if edge else [I, Q, wf.cos(2 * np.pi * f) * (wf.square(1e-6) >> t_center)]
    return chans, ('linspace', t_center - 1e-6, t_center + 1e-6, 40001, False)


def _flat_tops(n=20):
    rng = np.random.default_rng(5)
    return [wl._tree_sum([(wf.square(40e-9, edge=8e-9) >> ((k + 0.5) * 60e-9)) * wf.cos(2 * np.pi * rng.uniform(-2e8, 2e8), rng.uniform(0, 6))
                          for k in range(n)])]


def _generic():        # erf edges + sinc: generic terms and the direct tier
    return [(wf.square(40e-9, edge=8e-9) >> 100e-9) * wf.cos(2 * np.pi * 90e6) + 0.1 * wf.sinc(2e8) * (wf.square(300e-9) >> 150e-9)]


def _jitter(n, span, seed=0):
    return np.sort(np.random.default_rng(seed).uniform(0, span, n))


FINE = ('linspace', 0.0, 6 * W, 50000, False)
FMUL = ('linspace', 0.0, 3e-6, 1_500_000, False)     # (at a tenth of the rate these envelopes are short-tier pieces)
BIG = 1_100_000        # time lists from 2^20 points on take the NS = 8 builds

# name -> (channels, grid description or None, time list or None, environment of the compile AND the name call)
PLANS = {
    'short_fam0': lambda: (_awg(), AWG, None, {}),
    'short_fam0_no_pk': lambda: (_awg(), AWG, None, {'WFK_SH_NO_PK': '1'}),
    'short_fam1': lambda: (_awg(wf.chirp(1e8, 2e8, 30e-9) >> 5e-6), AWG, None, {}),
    'short_fam2': lambda: ([_pulse_train(lambda k, r: wf.square(36e-9, edge=3e-9) * wf.cos(2 * np.pi * r.uniform(-2e8, 2e8), r.uniform(0, 6)), 150, 60e-9)], AWG, None, {}),
    'short_fam4': lambda: (_awg(wf.chirp(1e8, 2e8, 30e-9, type='exponential') >> 5e-6), AWG, None, {}),
    'short_fam6': lambda: _corr_short() + (None, {}),
    'short_general': lambda: (_awg((wf.sinc(2e8) * wf.square(30e-9)) >> 5e-6), AWG, None, {}),
    'short_slice': lambda: (_awg(), ('slice', AWG, 3000, 9000), None, {}),
    'awg_cases_cplx': lambda: ([cases.AWG_CASES['cplx_2g'][0](wf, 2e9)], cases._awg_grid(cases.AWG_CASES['cplx_2g'][2], 2e9), None, {}),
    'lean_fam0': lambda: ([wl.sum_channel(wf, 6, 1000 + c) for c in range(2)], FINE, None, {}),
    'lean_fam1': lambda: ([wl.multitone_channel(wf, 0, ntones=4, nseg=6)], FINE, None, {}),
    'lean_fam2': lambda: ([(wf.chirp(1e8, 2e8, 300e-9) >> 100e-9) + (wf.gaussian(20e-9) >> 50e-9)], ('linspace', 0.0, 500e-9, 50000, False), None, {}),
    'lean_fam3': lambda: ([wl.direct_channel(wf, 'interp'), wl.direct_channel(wf, 'mollifier')], FMUL, None, {}),
    'lean_fam4': lambda: ([_pulse_train(lambda k, r: _hann(300 + k) * wf.cos(2 * np.pi * r.uniform(-2e8, 2e8), r.uniform(0, 6)), 60, 50e-9)
                           + 0.1 * _pulse_train(lambda k, r: _hann(64, 0.8) * wf.cos(2 * np.pi * r.uniform(-2e8, 2e8)), 55, 54e-9, 7e-9)], FMUL, None, {}),
    'lean_corr0': lambda: _far()[:1] + (_far()[1], None, {}),
    'lean_corr1': lambda: _far(edge=True)[:1] + (_far()[1], None, {}),
    'lean_general': lambda: ([((_hann() * (wf.cos(2e9) + wf.cos(2.5e9))) >> 1e-6) + (_hann(100) >> 1.004e-6)], FMUL, None, {}),
    'lean_slice': lambda: ([wl.sum_channel(wf, 6, 1000)], ('slice', FINE, 12345, 40000), None, {}),
    'readme_x': lambda: ([cases.CASES['readme_x'][0](wf)], ('linspace', -1e-6, 9e-6, 10001, True), None, {}),
    'general_plain': lambda: ([wl.sum_channel(wf, 6, 1000)], FINE, None, {'WFK_DISABLE_LEAN': '1'}),
    'general_generic': lambda: PLANS['lean_general']()[:3] + ({'WFK_DISABLE_MIXED': '1'},),
    'general_direct': lambda: (_generic(), ('linspace', 0.0, 300e-9, 25003, False), None, {}),
    'general_slice': lambda: (_generic(), ('slice', ('linspace', 0.0, 300e-9, 25003, False), 5001, 20000), None, {}),
    'grid_as_tlist': lambda: ([_pulse_train(lambda k, r: wf.sinc(6 / W) * wf.square(W) * wf.cos(2 * np.pi * r.uniform(-2e8, 2e8)), 300, W)], AWG, None, {}),
    'tlist_fused_small': lambda: ([wl.sum_channel(wf, 6, 1000)], None, _jitter(5001, 6 * W), {}),
    'tlist_full_small': lambda: ([wl.sum_channel(wf, 6, 1000)], None, _jitter(5001, 6 * W), {'WFK_DISABLE_TLFUSE': '1'}),
    'tlist_mixed_small': lambda: (_flat_tops(), None, _jitter(5001, 1.2e-6, 5), {}),
    'tlist_fused_big': lambda: ([wl.sum_channel(wf, 6, 1000)], None, _jitter(BIG, 6 * W), {}),
    'tlist_full_big': lambda: ([wl.sum_channel(wf, 6, 1000)], None, _jitter(BIG, 6 * W), {'WFK_DISABLE_TLFUSE': '1'}),
    'tlist_mixed_big': lambda: (_flat_tops(), None, _jitter(BIG, 1.2e-6, 5), {}),
}


def _grid(desc):
    if desc[0] == 'slice':
        return _flatten.grid_slice(_flatten.grid_from_desc(desc[1]), desc[2], desc[3])
    return _flatten.grid_from_desc(desc)


def names_of(key):
    chans, grid, t, env = PLANS[key]()
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        plan = _engine.Plan(_flatten.flatten(chans), grid=None if grid is None else _grid(grid), t=t)
        return [plan.kernel_name(dt) for dt in DTYPES]
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.update({k: v})


def record(path):
    with open(path, 'w') as f:
        json.dump({k: names_of(k) for k in sorted(PLANS)}, f, indent=1)
        f.write('\n')


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_plan_has_a_record(recorded):
    assert sorted(recorded) == sorted(PLANS)


@pytest.mark.parametrize('key', sorted(PLANS))
def test_kernel_names_are_what_they_were(key, recorded):
    assert names_of(key) == recorded[key]
