"""Host referees for `waveforms_amd.distortion.phase_curve` (shared by test_phase_curve_cpu.py and
test_gpu_phase_curve.py; NumPy / SciPy only, no device, no reference sources).

`restated` is the reference's phase_curve (waveforms/distortion.py:349-366) in this module's own words, with its
arithmetic: the filters of `distort` (:340-346) combined into one (b, a) (:226-244) and run by lfilter from the
lfiltic state of an all-zero history (:306-321), np.convolve(..., 'same') (:358-365), np.interp (:366).
`longdouble_curve` is the same curve with the filter as a CASCADE of first-order sections and every sum in
np.longdouble -- what three and four time constants are compared with, where the combined direct form in double is
itself 5e-10 .. 5e-5 off.  `combined_longdouble_curve` runs the combined (b, a) in np.longdouble: the distance of
`restated` from it is the `self_err` of the project's IIR bound max(1e-9 * scale, 10 * self_err)."""
import numpy as np
from scipy.signal import lfilter, lfiltic

from waveforms_amd.distortion import combine_filters, exp_decay_filter

LD = np.longdouble


def grid(t, sample_rate):
    """distortion.py:350-352 -> (lim, num, tlist)"""
    lim = max(np.max(np.abs(t)), 20e-6)
    num = round(2 * lim * sample_rate)
    return lim, num, np.arange(num) / sample_rate - lim


def kernel_points(pulse_width, start, sample_rate):
    """distortion.py:355-356 -> (pulse points, start points)"""
    return round(pulse_width * sample_rate), round((start + pulse_width) * sample_rate) - 1


def sections(params, sample_rate):
    return [exp_decay_filter(amp, abs(tau), sample_rate) for amp, tau in np.asarray(params).reshape(-1, 2)]


def distort_host(x, params, sample_rate):
    """distortion.py:340-346 with initial = 0: lfilter over the combined (b, a), from lfiltic's state for zero histories"""
    b, a = combine_filters(sections(params, sample_rate))
    zi = lfiltic(b, a, np.full((len(a) - 1, ), 0.0), np.full((len(b) - 1, ), 0.0))
    return lfilter(b, a, x, zi=zi)[0]


def restated(t, params, df_dphi, pulse_width, start, wav, sample_rate):
    _, _, tlist = grid(t, sample_rate)
    pp, sp = kernel_points(pulse_width, start, sample_rate)
    ker = np.hstack([np.ones(pp) / sample_rate, np.zeros(sp)])
    conv = np.convolve(2 * np.pi * df_dphi * distort_host(wav(tlist), params, sample_rate), ker, mode='same')
    return np.interp(t, tlist, conv)


def _first_order_ld(b, a, x):
    """one first-order section from rest in long double: y[i] = b0 x[i] + b1 x[i-1] - a1 y[i-1]"""
    b = np.concatenate([np.asarray(b, dtype=LD), np.zeros(2, dtype=LD)])[:2] / LD(a[0])
    a1 = (LD(a[1]) / LD(a[0])) if len(a) > 1 else LD(0)
    u = b[0] * x
    u[1:] += b[1] * x[:-1]
    y = np.empty(len(x), dtype=LD)
    prev = LD(0)
    for i in range(len(x)):
        prev = u[i] - a1 * prev
        y[i] = prev
    return y


def _direct_ld(b, a, x):
    """the lfilter recurrence (direct form II transposed) of one (b, a) from rest in long double"""
    m = max(len(a), len(b)) - 1
    bb, aa = np.zeros(m + 1, dtype=LD), np.zeros(m + 1, dtype=LD)
    bb[:len(b)] = np.asarray(b, dtype=LD) / LD(a[0])
    aa[:len(a)] = np.asarray(a, dtype=LD) / LD(a[0])
    if m == 0:
        return bb[0] * x
    z = np.zeros(m, dtype=LD)
    y = np.empty(len(x), dtype=LD)
    for i in range(len(x)):
        xx = x[i]
        yy = bb[0] * xx + z[0]
        for k in range(m - 1):
            z[k] = bb[k + 1] * xx - aa[k + 1] * yy + z[k + 1]
        z[m - 1] = bb[m] * xx - aa[m] * yy
        y[i] = yy
    return y


def _probe_ld(y, t, tlist, pp, sp, gain):
    """box sum of pp samples ending at i + c (zero padded) and linear interpolation with np.interp's brackets, in
    long double -> float64, shaped like t"""
    n, c = len(y), (pp + sp - 1) // 2
    cs = np.concatenate([np.zeros(1, dtype=LD), np.cumsum(y)])

    def conv(i):
        hi = np.clip(i + c + 1, 0, n)
        lo = np.clip(i + c - pp + 1, 0, n)
        return LD(gain) * (cs[np.maximum(hi, lo)] - cs[lo])

    tq = np.asarray(t, dtype=np.float64)
    j = np.clip(np.searchsorted(tlist, tq.reshape(-1), side='right') - 1, 0, n - 2)
    x0, x1 = tlist[j].astype(LD), tlist[j + 1].astype(LD)
    f0, f1 = conv(j), conv(j + 1)
    tc = np.clip(tq.reshape(-1), tlist[0], tlist[-1]).astype(LD)
    out = f0 + (f1 - f0) / (x1 - x0) * (tc - x0)
    return out.astype(np.float64).reshape(tq.shape)


def longdouble_curve(t, params, df_dphi, pulse_width, start, wav, sample_rate):
    _, _, tlist = grid(t, sample_rate)
    pp, sp = kernel_points(pulse_width, start, sample_rate)
    y = np.asarray(wav(tlist), dtype=np.float64).astype(LD)
    for b, a in sections(params, sample_rate):
        y = _first_order_ld(b, a, y)
    return _probe_ld(y, t, tlist, pp, sp, 2 * np.pi * df_dphi / sample_rate)


def combined_longdouble_curve(t, params, df_dphi, pulse_width, start, wav, sample_rate):
    _, _, tlist = grid(t, sample_rate)
    pp, sp = kernel_points(pulse_width, start, sample_rate)
    b, a = combine_filters(sections(params, sample_rate))
    y = _direct_ld(b, a, np.asarray(wav(tlist), dtype=np.float64).astype(LD))
    return _probe_ld(y, t, tlist, pp, sp, 2 * np.pi * df_dphi / sample_rate)


def scale(want):
    return max(1.0, float(np.max(np.abs(want))))


def demo_wave_host(t):
    """the demo's wave, 0.1 * (square(2e-6) << 1e-6) (distortion.py:381), as a plain NumPy step: 0.1 on [-2 us, 0)"""
    t = np.asarray(t)
    return np.where((t >= -2e-6) & (t < 0), 0.1, 0.0)


DF_DPHI = 4343.313e6                                   # distortion.py:378
# delays inside the 2 us pulse (where the phase is of the order of 2 pi df_dphi * 0.1 * 10 ns = 27) and after it
DEMO_T = np.concatenate([np.linspace(-2.5e-6, -5e-9, 20), np.geomspace(5e-9, 15e-6, 40)])
# the demo's kernels (distortion.py:384, 392-398) and a long pulse, with one and two time constants
DEMO_CASES = [(params, pw, start)
              for params in ([-0.03, 0.1e-6], [-0.03, 0.1e-6, 0.02, 0.3e-6])
              for pw, start in ((10e-9, 25e-9), (10e-9, 0.0), (500e-9, 25e-9))]
