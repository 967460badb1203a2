"""Referee of the per-row IIR stage that ends in DAC codes (distortion.IirDacStage / iir_dac_rows,
csrc/wfk_iir_rows_dac.hip): `dac_rows_ref.dac_ref` of the per-row lfilter as tests/test_gpu_iir_rows.py forms it (scipy,
section after section, from the row's zi, around the row's level), and the inputs the CPU and the GPU tests share.

The device IIR is not bit-equal to lfilter: it is held to tol_y = max(1e-9 * scale, 10 * self_err) (self_err: the
referee's own distance from the np.longdouble recurrence, scale = max(1, |y|.max())), the bound of
tests/test_gpu_iir_rows.py.  A code may therefore differ from the referee's only at an UNDECIDED sample: one whose
referee v = y * gain + offset lies within delta = |gain| * tol_y (+ the two roundings of v) of a half-integer -- the
rails' rounding boundaries lo - 0.5 and hi + 0.5 are half-integers too -- and there by one step.  `undecided` marks
them from the referee alone."""
import numpy as np
from scipy.signal import lfilter

import dac_rows_ref

SHAPES = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (3, 1), (4, 1), (2, 2)]      # (n_sections, order): iir_rows_tile's
FORMATS = [(16, 0), (14, 2), (2, 14)]                                          # (bits, shift)
LENGTHS = [1, 7, 8, 9, 16, 17, 4095, 4096, 4097, 12000]    # one lane, a slot edge, a run edge, a tile edge, two tiles and a part
BATCHES = [1, 3, 17]
TILE = 4096
MAX_UNDECIDED_SHARE = 1e-3


def random_rows(rng, batch, nsec, order):
    """per row: nsec sections of the given order, real poles in 0.3 .. 0.97 (well conditioned), a[0] != 1 -- the rows
    of tests/test_gpu_iir_rows.py::_random_rows"""
    rows = []
    for _ in range(batch):
        secs = []
        for _ in range(nsec):
            a = np.poly(rng.uniform(0.3, 0.97, order) * rng.choice([-1, 1], order, p=[0.2, 0.8]))
            b = rng.uniform(-1, 1, order + 1)
            a0 = rng.uniform(0.5, 2.0)
            secs.append((b * a0, a * a0))
        rows.append(secs)
    return rows


def cascade(secs, x, zi, initial=0.0):
    """scipy, section after section, around the row's level; zi: the sections' states back to back -> (y, zf)"""
    zf, pos, x = [], 0, np.asarray(x, dtype=np.float64) - initial
    for b, a in secs:
        m = max(len(a), len(b)) - 1
        x, z = lfilter(b, a, x, zi=zi[pos:pos + m])
        zf.append(z)
        pos += m
    return x + initial, np.concatenate(zf)


def _lfilter_longdouble(b, a, x, zi):
    """the lfilter recurrence (direct form II transposed) in np.longdouble, its result left in long double"""
    ld = np.longdouble
    m = max(len(a), len(b)) - 1
    bb, aa = np.zeros(m + 1, dtype=ld), np.zeros(m + 1, dtype=ld)
    bb[:len(b)] = np.asarray(b, dtype=ld) / ld(a[0])
    aa[:len(a)] = np.asarray(a, dtype=ld) / ld(a[0])
    z = np.asarray(zi, dtype=ld).copy()
    y = np.empty(len(x), dtype=ld)
    for t in range(len(x)):
        xx = x[t]
        yy = bb[0] * xx + z[0]
        for j in range(m - 1):
            z[j] = bb[j + 1] * xx - aa[j + 1] * yy + z[j + 1]
        z[m - 1] = bb[m] * xx - aa[m] * yy
        y[t] = yy
    return y


def cascade_longdouble(secs, x, zi, initial=0.0):
    pos, x = 0, np.asarray(x, dtype=np.longdouble) - np.longdouble(initial)
    for b, a in secs:
        m = max(len(a), len(b)) - 1
        x = _lfilter_longdouble(b, a, x, zi[pos:pos + m])
        pos += m
    return (x + np.longdouble(initial)).astype(np.float64)


def gains_offsets(y, bits, seed):
    """per row of the referee's y: a gain whose sign alternates from row to row and which puts the rails 1.2 standard
    deviations from the row's mean (a row of a few samples: at half its largest deviation), and an offset that centres
    the row between them plus a fraction of an LSB -- so that rows clip on both rails"""
    rng = np.random.default_rng(seed)
    half = 2.0**(bits - 1)                                 # the rails' rounding boundaries are -0.5 +- half
    y = np.asarray(y, dtype=np.float64)
    mean = y.mean(axis=1)
    dev = y - mean[:, None]
    spread = 1.2 * dev.std(axis=1) if y.shape[1] >= 64 else 0.5 * np.abs(dev).max(axis=1)
    gain = half / np.maximum(spread, 1e-3) * np.where(np.arange(len(y)) % 2 == 0, 1.0, -1.0)
    offset = -gain * mean - 0.5 + rng.uniform(-0.45, 0.45, len(y))
    return gain, offset


class Case:
    """one batch: cascades, input, zi, levels, the referee's y and zf, and a gain / offset per row for `bits`"""

    def __init__(self, nsec, order, batch, n, bits=16, shift=0, seed=None, dtype=np.float64):
        self.nsec, self.order, self.batch, self.n, self.bits, self.shift = nsec, order, batch, n, bits, shift
        self.seed = 1000 * nsec + 100 * order + 7 * batch + n % 97 if seed is None else seed
        rng = np.random.default_rng(self.seed)
        self.rows = random_rows(rng, batch, nsec, order)
        self.x = rng.standard_normal((batch, n)).astype(dtype)
        self.zi = rng.standard_normal((batch, nsec * order)) * 0.2
        self.initial = np.round(rng.uniform(-0.5, 0.5, batch), 3)
        both = [cascade(self.rows[r], self.x[r], self.zi[r], self.initial[r]) for r in range(batch)]
        self.y = np.stack([b[0] for b in both])
        self.zf = np.stack([b[1] for b in both])
        self.gain, self.offset = gains_offsets(self.y, bits, self.seed + 1)

    def reference(self):
        """-> (codes, counts) of the referee"""
        return dac_rows_ref.dac_ref(self.y, self.gain, self.offset, self.bits, self.shift)

    def tol_y(self):
        """per row: max(1e-9 * scale, 10 * self_err)"""
        out = np.empty(self.batch)
        for r in range(self.batch):
            exact = cascade_longdouble(self.rows[r], self.x[r], self.zi[r], self.initial[r])
            self_err = float(np.max(np.abs(self.y[r] - exact))) if self.n else 0.0
            out[r] = max(1e-9 * max(1.0, float(np.abs(self.y[r]).max(initial=0.0))), 10 * self_err)
        return out

    def undecided(self, tol_y=None):
        """-> (mask (batch, n) of the undecided samples, near_lo, near_hi: those of them at the rails' boundaries)"""
        tol_y = self.tol_y() if tol_y is None else tol_y
        lo, hi = dac_rows_ref.rails(self.bits)
        v = self.y * self.gain[:, None] + self.offset[:, None]
        delta = np.abs(self.gain)[:, None] * tol_y[:, None] + 2.0**-50 * np.maximum(1.0, np.abs(v))
        frac = np.abs(v - np.floor(v) - 0.5)                          # distance from the nearest half-integer
        mask = frac <= delta
        return mask, mask & (np.abs(v - (lo - 0.5)) <= delta), mask & (np.abs(v - (hi + 0.5)) <= delta)


def referee_cases():
    """the batches the GPU test holds against the referee (float64; the undecided share of each, from the referee
    alone, is held to MAX_UNDECIDED_SHARE by tests/test_iir_dac_cpu.py): every shape over two tiles and a sample, and
    the order-3 section over two tiles and a part in the two narrower formats"""
    out = [Case(nsec, order, 3, TILE + 1) for nsec, order in SHAPES]
    out += [Case(1, 3, 3, 12000, bits, shift) for bits, shift in FORMATS[1:]]
    return out
