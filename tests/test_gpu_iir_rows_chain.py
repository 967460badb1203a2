"""The sampler inside the per-row IIR stage (csrc/wfk_iir_rows_sampled.hip): `distortion.SampledIirRows`, the raw
`_engine.ChainIirRowsPlan` and the plain-C consumer tests/c_abi/chain_iir_rows_smoke.c.

Reference: the C oracle's samples (`c_oracle.eval_grid`, pinned to reference-generated goldens) filtered the
reference's way, row by row: SciPy's lfilter section after section on x - initial, + initial (`_cascade`, the form of
tests/test_gpu_iir_chain.py).  Tolerances are the project's own (tests/cases.py, tests/test_gpu_iir_rows.py):
FP64_IIR_TOL * scale for outputs, 1e-10 * scale for zf, FP32_TOL * scale for float rows, scale = max(1, |want|.max());
for a row given as ONE combined (b, a) of order 3, max(1e-9 * scale, 10 * self_err), self_err the reference's own
distance from the np.longdouble recurrence.  Every row used is admitted only if the reference is trustworthy on it,
self_err < 1e-10 * max(1, peak): `test_rows_are_well_conditioned` asserts that for all of them, none is dropped.

Every fused case asserts `.fused` and the kernel-name prefix: none can pass through the fallback."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy.signal import butter, lfilter

from cases import FP32_TOL, FP64_IIR_TOL
import row_windows
import waveforms_amd as wf
from oracle import c_oracle
from waveforms_amd import _flatten, workloads as wl
from waveforms_amd.distortion import SampledIirRows, combine_filters, exp_decay_filter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = FP64_IIR_TOL
TILE = 4096                 # samples a workgroup evaluates and filters per step
N_AWG = 12000               # two whole tiles and a partial one
N_FINE = 12001              # the fine grid: 6 pulses of ~2000 samples, their edges inside the tiles
FILLS = ('short', 'lean')
PREFIX = {'short': 'iir_rows_short<', 'lean': 'iir_rows_sampled<'}

# (amp, tau) of the first-order exp-decay sections; the cascades of the issue's conditioning table
TC4 = [(0.01, 20e-9), (0.02, 200e-9), (-0.015, 1e-6), (0.01, 5e-6)]
TC3 = [(0.03, 40e-9), (0.01, 900e-9), (-0.005, 5e-6)]
TC2 = [(-0.02, 80e-9), (-0.01, 1.5e-6)]
TC1 = [(0.02, 150e-9)]
TC_ORDER3 = [(0.015, 20e-9), (0.01, 50e-9), (-0.02, 150e-9)]     # combined into ONE (b, a) of order 3
ROW_TCS = [TC1, TC2, TC3, TC4, TC4[:2]]                          # 1, 2, 3, 4 and 2 sections: the padding path
ROW_INITIAL = np.array([0.0, 0.3, -0.2, 0.1, 0.5])


def _secs(tcs, rate):
    return [exp_decay_filter(A, tau, rate) for A, tau in tcs]


def _rate(fill):
    """the rate the exp-decay sections are designed for: 2 GS/s on both fills -- a row's filter is its coefficients, and
    designed for the fine grid's own 67 GS/s the poles would sit where the reference itself is 1e-8 off"""
    return 2e9


def _shapes(rate):
    """one cascade per (NSEC, ORD) instantiation: SHAPES of tests/test_gpu_iir_chain.py plus 2 and 3 first-order
    sections and the combined order 3 of the conditioning table"""
    return {
        'biquad': [(r[:3], r[3:]) for r in butter(2, 0.04, output='sos')],                   # (1, 2)
        'two_biquads': [(r[:3], r[3:]) for r in butter(4, 0.03, output='sos')],              # (2, 2)
        'first_order': _secs(TC1, rate),                                                     # (1, 1)
        'two_first_order': _secs(TC2, rate),                                                 # (2, 1)
        'three_first_order': _secs(TC3, rate),                                               # (3, 1)
        'four_first_order': _secs(TC4, rate),                                                # (4, 1)
        'order3': [butter(3, 0.05)],                                                         # (1, 3)
        'order3_combined': [combine_filters(_secs(TC_ORDER3, rate))],                        # (1, 3)
        'order4': [butter(4, 0.08)],                                                         # (1, 4)
    }


NSEC_ORD = {'biquad': (1, 2), 'two_biquads': (2, 2), 'first_order': (1, 1), 'two_first_order': (2, 1),
            'three_first_order': (3, 1), 'four_first_order': (4, 1), 'order3': (1, 3), 'order3_combined': (1, 3),
            'order4': (1, 4)}


def _channels(fill, rows=5, n=None):
    if fill == 'short':
        return [wl.awg_channel(wf, c, N_AWG if n is None else n, 2e9) for c in range(rows)]
    return [wl.sum_channel(wf, 6, 1000 + c) for c in range(rows)]


def _grid(fill, n=None):
    """the fill's grid as a wfk_grid; n: its first n samples (the same step)"""
    g = _flatten.grid_from_desc(wl.awg_grid(N_AWG, 2e9) if fill == 'short'
                                else ('linspace', 0.0, 6 * wl.SPAN, N_FINE, False))
    return g if n is None else _flatten.grid_slice(g, 0, n)


def _cascade(sections, x, initial=0.0, zi=None):
    """the reference's filtering of one row: sections one after the other on x - initial, + initial; -> (y, zf)"""
    y = np.asarray(x, dtype=np.float64) - initial
    zf, off = [], 0
    for b, a in sections:
        m = max(len(b), len(a)) - 1
        z0 = np.zeros(m) if zi is None else np.asarray(zi[off:off + m], dtype=np.float64)
        y, z1 = lfilter(b, a, y, zi=z0)
        zf.append(z1)
        off += m
    return y + initial, np.concatenate(zf)


def _longdouble_cascades(jobs):
    """jobs: [(sections, x, initial)] -> [y]: the cascades' recurrence (direct form II transposed, zero state, on
    x - initial, + initial) in np.longdouble, all jobs stepped together (one Python loop over the samples per stage)"""
    ld = np.longdouble
    ys = [np.asarray(x, dtype=ld) - ld(ini) for _, x, ini in jobs]
    for stage in range(max(len(secs) for secs, _, _ in jobs)):
        live = [j for j, (secs, _, _) in enumerate(jobs) if len(secs) > stage]
        order = lambda j: max(len(jobs[j][0][stage][0]), len(jobs[j][0][stage][1])) - 1
        for m, n in sorted({(order(j), len(ys[j])) for j in live}):      # jobs of one section order and row length together
            idx = [j for j in live if (order(j), len(ys[j])) == (m, n)]
            bb, aa = np.zeros((len(idx), m + 1), dtype=ld), np.zeros((len(idx), m + 1), dtype=ld)
            for k, j in enumerate(idx):
                sb, sa = jobs[j][0][stage]
                bb[k, :len(sb)] = np.asarray(sb, dtype=ld) / ld(sa[0])
                aa[k, :len(sa)] = np.asarray(sa, dtype=ld) / ld(sa[0])
            x = np.stack([ys[j] for j in idx])
            y = np.empty_like(x)
            z = np.zeros((len(idx), m), dtype=ld)
            for t in range(x.shape[1]):
                xx = x[:, t]
                yy = bb[:, 0] * xx + z[:, 0]
                for i in range(m - 1):
                    z[:, i] = bb[:, i + 1] * xx - aa[:, i + 1] * yy + z[:, i + 1]
                z[:, m - 1] = bb[:, m] * xx - aa[:, m] * yy
                y[:, t] = yy
            for k, j in enumerate(idx):
                ys[j] = y[k]
    return [(y + ld(ini)).astype(np.float64) for y, (_, _, ini) in zip(ys, jobs)]


def _scale(want):
    return max(1.0, float(np.abs(want).max()))


# ---- the configurations the tests below filter: (channels, grid, one cascade per row, one level per row)
def cfg_rows(fill, rate=None):
    """the parity rows: 5 AWG rows (1, 2, 3, 4 and 2 sections) / 3 fine-grid rows, a level per row"""
    if fill == 'short':
        rate = 2e9 if rate is None else rate
        return ([wl.awg_channel(wf, c, N_AWG, rate) for c in range(5)], _flatten.grid_from_desc(wl.awg_grid(N_AWG, rate)),
                [_secs(tc, rate) for tc in ROW_TCS], ROW_INITIAL)
    return _channels('lean', 3), _grid('lean'), [_secs(tc, _rate('lean')) for tc in ROW_TCS[:3]], ROW_INITIAL[:3]


def cfg_shape(fill, shape):
    secs = _shapes(_rate(fill))[shape]
    return _channels(fill, 2), _grid(fill), [secs, secs], np.zeros(2)


def cfg_edge(fill):
    """a constant offset and a `>>` shift"""
    a, b = _channels(fill, 2)
    return [a + 0.25, b >> 7e-9], _grid(fill), [_secs(TC2, _rate(fill)), _secs(TC1, _rate(fill))], np.array([0.25, -0.1])


def cfg_clip_short():
    """AWG-rate rows with Waveform.min / .max set: the short fill clips its runs itself (before the channel offset)"""
    chans = _channels('short', 2)
    chans[0].max, chans[0].min = 0.4, -0.3
    chans[1].max, chans[1].min = 0.05, -0.6
    return chans, _grid('short'), [_secs(TC2, 2e9), _secs(TC3, 2e9)], np.array([0.1, -0.2])


def cfg_fallback(kind):
    base, rate = wl.sum_channel(wf, 6, 11), _rate('lean')
    other = wl.sum_channel(wf, 6, 12)
    if kind == 'clip':
        other.max, other.min = 0.4, -0.3
    chans = {'clip': [base, other], 'complex': [base * (1 + 0.5j), other], 'fused': [wf.sinc(40e6) >> 3 * wl.SPAN, other]}[kind]
    return chans, _grid('lean'), [_secs(TC2, rate), _secs(TC1, rate)], np.array([0.1, 0.1])


CONFIGS = [('rows', f, r) for f, r in (('short', 1e9), ('short', 2e9), ('lean', None))] + \
          [('shape', f, sh) for f in FILLS for sh in sorted(NSEC_ORD)] + [('edge', f) for f in FILLS] + \
          [('fallback', k) for k in ('clip', 'complex', 'fused')] + [('clip_short', )]


@functools.lru_cache(maxsize=None)
def _config(key):
    """-> (channels, grid, cascades, levels, the oracle's samples on the grid (real part), computed once and left alone)"""
    chans, grid, secs, ini = {'rows': cfg_rows, 'shape': cfg_shape, 'edge': cfg_edge, 'fallback': cfg_fallback,
                             'clip_short': cfg_clip_short}[key[0]](*key[1:])
    x = np.ascontiguousarray(c_oracle.eval_grid(_flatten.flatten(chans), grid).real)
    x.setflags(write=False)
    return chans, grid, secs, ini, x


@functools.lru_cache(maxsize=None)
def _self_errs():
    """{(config key, row): distance of the reference (lfilter in double, section after section) from the long-double
    recurrence}, for every row of every configuration"""
    keys, jobs = [], []
    for key in CONFIGS:
        _, _, secs, ini, x = _config(key)
        for r in range(len(secs)):
            keys.append((key, r))
            jobs.append((secs[r], x[r], float(ini[r])))
    exact = _longdouble_cascades(jobs)
    return {k: float(np.max(np.abs(_cascade(s, x, i)[0] - e))) for k, (s, x, i), e in zip(keys, jobs, exact)}


def test_rows_are_well_conditioned():
    """every row used passes self_err < 1e-10 * max(1, peak): an assertion, not a filter"""
    for (key, r), err in _self_errs().items():
        print(f'{key} row {r}: self_err {err:.3g}')
        assert err < 1e-10 * max(1.0, float(np.abs(_config(key)[4][r]).max())), (key, r, err)


def _check(sr, want, wzf, got, zf, tol=TOL, ztol=1e-10, what=''):
    ey = np.max(np.abs(got - want)) / _scale(want) if want.size else 0.0
    ez = np.max(np.abs(zf - wzf)) / _scale(wzf) if zf is not None and wzf.size else 0.0
    print(f'{what} {sr.kernel_name()}: y {ey:.3g} zf {ez:.3g} of scale (tol {tol:.3g} / {ztol:.3g})')
    assert ey <= tol and ez <= ztol, (what, ey, ez)


def _fused(sr, fill):
    assert sr.fused, sr.why_not
    assert sr.kernel_name().startswith(PREFIX[fill]), sr.kernel_name()
    assert sr.why_not == ''


def _check_rows(sr, key, got, zf, lo=0, hi=None, tol=TOL, ztol=1e-10, zi=None):
    """every row of a configuration (its samples lo .. hi) against the reference"""
    _, _, secs, ini, x = _config(key)
    for r in range(len(secs)):
        want, wzf = _cascade(secs[r], x[r, lo:hi], ini[r], None if zi is None else zi[r])
        _check(sr, want, wzf, got[r], None if zf is None else sr.row_state(zf, r), tol, ztol, f'{key} row {r}')


# ---- 1, 2: parity of the two fills, per-row cascades of mixed section counts, per-row initial, zf through row_state
@pytest.mark.parametrize('rate', [1e9, 2e9])
def test_short_fill_parity(rate):
    key = ('rows', 'short', rate)
    chans, grid, secs, ini, _ = _config(key)
    sr = SampledIirRows(chans, grid, secs)
    _fused(sr, 'short')
    assert sr.kernel_name() == 'iir_rows_short<f64,4,1>' and sr.state_dim == 4 and (sr.n, sr.n_channels) == (N_AWG, 5)
    assert sr.own_orders == [[1] * len(tc) for tc in ROW_TCS] and sr.section_order == 1
    got, zf = sr.to_host(initial=ini, return_zf=True)
    _check_rows(sr, key, got, zf)
    for r in range(5):
        assert not zf[r, len(ROW_TCS[r]):].any()                  # the padding sections keep a zero state
    sr.close()


def test_lean_fill_parity():
    key = ('rows', 'lean', None)
    chans, grid, secs, ini, _ = _config(key)
    sr = SampledIirRows(chans, grid, secs)
    _fused(sr, 'lean')
    assert sr.kernel_name() == 'iir_rows_sampled<f64,3,1>' and sr.state_dim == 3
    got, zf = sr.to_host(initial=ini, return_zf=True)
    _check_rows(sr, key, got, zf)
    sr.close()


def test_short_fill_clips_its_runs():
    """clipped channels at AWG rates stay fused (only the lean fill refuses clip)"""
    key = ('clip_short', )
    chans, grid, secs, ini, x = _config(key)
    assert x[0].max() == 0.4 and x[0].min() == -0.3 and x[1].max() == 0.05      # the clip bites
    sr = SampledIirRows(chans, grid, secs)
    _fused(sr, 'short')
    got, zf = sr.to_host(initial=ini, return_zf=True)
    _check_rows(sr, key, got, zf)
    sr.close()


# ---- 3: every (NSEC, ORD) instantiation on both fills
@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('shape', sorted(NSEC_ORD))
def test_every_shape_on_both_fills(fill, shape):
    key = ('shape', fill, shape)
    chans, grid, secs, _, x = _config(key)
    sr = SampledIirRows(chans, grid, secs)
    _fused(sr, fill)
    assert sr.kernel_name() == PREFIX[fill] + 'f64,%d,%d>' % NSEC_ORD[shape]
    got, zf = sr.to_host(return_zf=True)
    for r in range(2):
        want, wzf = _cascade(secs[r], x[r])
        tol = TOL
        if shape == 'order3_combined':       # the reference itself is 3e-12 .. 1.3e-11 off the long-double recurrence here
            tol = max(1e-9 * _scale(want), 10 * _self_errs()[(key, r)]) / _scale(want)
        _check(sr, want, wzf, got[r], zf[r], tol=tol, what=f'{fill} {shape} row {r}')
    sr.close()


# ---- 4: tail and edge lengths, an offset and a shift
@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('n', [1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193])
def test_tail_and_edge_lengths(fill, n):
    key = ('edge', fill)
    chans, grid, secs, ini, _ = _config(key)
    sr = SampledIirRows(chans, _flatten.grid_slice(grid, 0, n), secs)
    _fused(sr, fill)
    got, zf = sr.to_host(initial=ini, return_zf=True)
    assert got.shape == (2, n)
    _check_rows(sr, key, got, zf, 0, n)
    sr.close()


@pytest.mark.parametrize('fill', FILLS)
def test_endpoint_grid_and_grid_slice(fill):
    """the overridden last sample of a linspace(endpoint=True) grid; a slice with i0 != 0 of the fill's grid"""
    key = ('edge', fill)
    chans, grid, secs, ini, _ = _config(key)
    n = int(grid.n)
    g = _flatten.grid_from_desc(('linspace', 0.0, (n - 1) * grid.step, n, True))
    assert g.has_last
    sr = SampledIirRows(chans, g, secs)
    _fused(sr, fill)
    x = c_oracle.eval_grid(_flatten.flatten(chans), g)
    got, zf = sr.to_host(initial=ini, return_zf=True)
    for r in range(2):          # (the rows of the configuration but for the last sample's time: conditioned as they are)
        want, wzf = _cascade(secs[r], x[r], ini[r])
        _check(sr, want, wzf, got[r], sr.row_state(zf, r), what=f'{fill} endpoint row {r}')
    sr.close()
    lo, hi = 3001, 3001 + 2 * TILE + 77
    sr = SampledIirRows(chans, _flatten.grid_slice(grid, lo, hi), secs)
    _fused(sr, fill)
    got, zf = sr.to_host(initial=ini, return_zf=True)
    _check_rows(sr, key, got, zf, lo, hi)
    sr.close()


# ---- 5: carried state, per-row initial as a device tensor
@pytest.mark.parametrize('fill', FILLS)
def test_carried_state_across_grid_slices(fill):
    key = ('rows', fill, 2e9 if fill == 'short' else None)
    chans, g, secs, levels, _ = _config(key)
    rows, n, cut = len(secs), int(g.n), 5000                          # the cut is not a tile multiple
    ini = torch.from_numpy(np.array(levels)).cuda()
    whole = SampledIirRows(chans, g, secs)
    _fused(whole, fill)
    out = torch.empty((rows, n), dtype=torch.float64, device='cuda')
    whole.launch_torch(out, initial=ini)
    parts, state = [], None
    for lo, hi in ((0, cut), (cut, n)):
        sh = SampledIirRows(chans, _flatten.grid_slice(g, lo, hi), secs)
        _fused(sh, fill)
        o = torch.empty((rows, hi - lo), dtype=torch.float64, device='cuda')
        zf = torch.zeros((rows, sh.state_dim), dtype=torch.float64, device='cuda')
        sh.launch_torch(o, initial=ini, zi=state, zf=zf)
        parts.append(o.cpu().numpy())
        state = zf
        sh.close()
    got = out.cpu().numpy()
    _check_rows(whole, key, got, None)
    whole.close()
    assert np.max(np.abs(np.concatenate(parts, axis=1) - got)) <= TOL * _scale(got)


# ---- 6: float rows
@pytest.mark.parametrize('fill', FILLS)
def test_float_rows(fill):
    key = ('rows', fill, 2e9 if fill == 'short' else None)
    chans, grid, secs, ini, _ = _config(key)
    sr = SampledIirRows(chans, grid, secs, dtype=np.float32)
    _fused(sr, fill)
    assert sr.kernel_name() == PREFIX[fill] + ('f32,4,1>' if fill == 'short' else 'f32,3,1>')
    got, zf = sr.to_host(initial=ini, return_zf=True)
    assert got.dtype == np.float32
    _check_rows(sr, key, got, zf, tol=FP32_TOL, ztol=FP32_TOL)
    sr.close()


# ---- 7: output windows
@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_rows_as_a_window_of_a_wider_tensor(fill, dtype):
    key = ('rows', fill, 2e9 if fill == 'short' else None)
    chans, grid, secs, ini, _ = _config(key)
    sr = SampledIirRows(chans, grid, secs, dtype=dtype)
    _fused(sr, fill)
    w = row_windows.Window(len(secs), sr.n, dtype)
    sr.launch_torch(w.win, initial=ini)
    torch.cuda.synchronize()
    w.assert_guards()
    _check_rows(sr, key, w.host(), None, tol=TOL if dtype is np.float64 else FP32_TOL)
    sr.close()


# ---- 8: reproducibility, independence of the position in the batch
@pytest.mark.parametrize('fill', FILLS)
def test_bitwise_reproducible_and_independent_of_the_batch(fill):
    key = ('rows', fill, 2e9 if fill == 'short' else None)
    chans, grid, secs, ini, _ = _config(key)
    sr = SampledIirRows(chans, grid, secs)
    _fused(sr, fill)
    a, za = sr.to_host(initial=ini, return_zf=True)
    b, zb = sr.to_host(initial=ini, return_zf=True)
    name = sr.kernel_name()
    sr.close()
    assert row_windows.bits_equal(a, b) and row_windows.bits_equal(za, zb)
    # the row with the most sections (alone it has the batch's padded shape, so the same instantiation runs): alone, and
    # at another position of a reordered batch
    top = max(range(len(secs)), key=lambda r: len(secs[r]))
    others = [r for r in range(len(secs)) if r != top]
    for order in ([top], others + [top] if top != len(secs) - 1 else [top] + others):
        s2 = SampledIirRows([chans[i] for i in order], grid, [secs[i] for i in order])
        _fused(s2, fill)
        assert s2.kernel_name() == name
        c, zc = s2.to_host(initial=np.asarray(ini)[order], return_zf=True)
        s2.close()
        at = order.index(top)
        assert row_windows.bits_equal(c[at], a[top]) and row_windows.bits_equal(zc[at], za[top]), (fill, order)


# ---- 9: fallbacks
def _fallback(key, word):
    chans, grid, secs, ini, _ = _config(key)
    sr = SampledIirRows(chans, grid, secs)
    assert not sr.fused and sr.why_not and word in sr.why_not, sr.why_not
    name = sr.kernel_name()
    assert name.startswith('wfk_sample') and ' + iir_rows_tile<f64,' in name and name.endswith('>'), name
    got, zf = sr.to_host(initial=ini, return_zf=True)
    _check_rows(sr, key, got, zf)
    sr.close()
    return got


@pytest.mark.parametrize('kind', ['clip', 'complex', 'fused'])
def test_plans_that_cannot_fuse_run_sampler_then_filter(kind):
    """a clipped channel on the fine grid; a complex channel; a generic term (sinc): 'not fully fused'"""
    _fallback(('fallback', kind), kind)


@pytest.mark.parametrize('fill', FILLS)
def test_the_unfused_switch(fill):
    key = ('rows', fill, 2e9 if fill == 'short' else None)
    chans, grid, secs, ini, _ = _config(key)
    sr = SampledIirRows(chans, grid, secs)
    _fused(sr, fill)
    fused = sr.to_host(initial=ini)
    sr.close()
    os.environ['WFK_CHAIN_UNFUSED'] = '1'
    try:
        got = _fallback(key, 'WFK_CHAIN_UNFUSED')
    finally:
        del os.environ['WFK_CHAIN_UNFUSED']
    assert np.max(np.abs(got - fused)) <= TOL * _scale(fused)


def test_empty_rows_launch_nothing():
    chans, grid, secs, _, _ = _config(('edge', 'short'))
    sr = SampledIirRows(chans, _flatten.grid_slice(grid, 0, 0), secs)
    assert sr.n == 0 and not sr.fused and sr.why_not
    out = torch.empty((2, 0), dtype=torch.float64, device='cuda')
    assert sr.launch_torch(out).shape == (2, 0)
    sr.close()


# ---- 10: the plain-C consumer
def test_plain_c_consumer_filters_on_the_device(tmp_path):
    exe = tmp_path / 'chain_iir_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'chain_iir_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    name = r.stdout.split('chain_iir_rows_smoke: ')[-1]
    assert 'parity ok' in r.stdout and name.startswith(('iir_rows_sampled<f64,1,1>', 'iir_rows_short<f64,1,1>')), r.stdout
