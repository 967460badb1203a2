"""Referee of the per-row curve + IIR stage that ends in DAC codes (distortion.CurveIirDacStage / curve_iir_dac_rows,
csrc/wfk_iir_rows_curve_dac.hip): `curve_rows_ref.curve_ref` / `counts_ref`, then `iir_dac_ref`'s cascade and
`dac_rows_ref.dac_ref`, and the inputs the CPU and the GPU tests share.  A plain module; nothing here touches a device.

The curve is bit-exact on the device (np.interp), the converter too; the IIR between them is held to iir_dac_ref's
tol_y.  So `beyond` is exact, and a code may differ from the referee's only at an UNDECIDED sample, as iir_dac_ref
spells it -- the referee's v within |gain| * tol_y of a half-integer -- and there by one step."""
import numpy as np

import curve_rows_ref as cref
import dac_rows_ref
import iir_dac_ref as iref

SHAPES, FORMATS, LENGTHS, BATCHES, TILE = iref.SHAPES, iref.FORMATS, iref.LENGTHS, iref.BATCHES, iref.TILE
MAX_UNDECIDED_SHARE = iref.MAX_UNDECIDED_SHARE
# knots whose range xp[-1] - xp[0] overflows: the plan gives the row no bucket table (plain bisection)
WIDE = (np.array([-1.5e308, -1.0, 0.5, 1.5e308]), np.array([-0.4, -0.2, 0.3, 0.5]))


def wide(xp):
    """does the range of the knots overflow"""
    with np.errstate(over='ignore'):
        return not np.isfinite(xp[-1] - xp[0])


def curve_pool():
    """the ragged batch of curve_rows_ref (K = 2, 1024 log-spaced, 65 uniform), then K = 33 and K = 1024 uniform,
    K = 33 log-spaced, and the row whose range overflows.  The values of all but the first are scaled by 4: volts of
    order one, the scale of iir_dac_ref's rows (its tol_y has an absolute floor: smaller rows would only raise the gains)"""
    xs, fs = cref.ragged_batch()
    more = [cref.knots(33, 'uniform'), cref.knots(1024, 'uniform'), cref.knots(33, 'log'), WIDE]
    xs, fs = xs + [m[0] for m in more], fs + [m[1] for m in more]
    return xs, fs[:1] + [4.0 * f for f in fs[1:]]


def curves_for(batch, first=0):
    """`batch` curves, the pool taken in turn from entry `first` on -> (xp_rows, fp_rows), lists"""
    xs, fs = curve_pool()
    pick = [(first + r) % len(xs) for r in range(batch)]
    return [xs[i] for i in pick], [fs[i] for i in pick]


def ends_for(batch, mode):
    """left / right: 'default' (None: the rows' end values), 'given' (finite, one per row), 'nan' (given, with NaN on
    the left of every second row -- a sample below the knots then poisons the row's state, as it does the two stages')"""
    if mode == 'default':
        return None, None
    r = np.arange(batch, dtype=np.float64)
    left, right = -0.35 - 0.01 * r, 0.45 + 0.02 * r
    if mode == 'nan':
        left[1::2] = np.nan
    return left, right


def input_row(n, xp, seed, dtype, specials):
    """curve_rows_ref.row_input; for the row whose range overflows, samples over [-2, 2] and -- `specials` -- NaN, +-inf
    and knots scattered over it"""
    if not wide(xp):
        return cref.row_input(n, xp, seed, dtype, specials)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, n)
    if specials and n:
        sp = np.array([np.nan, np.inf, -np.inf, -1.0, 0.5, 0.0, np.nextafter(-1.0, 0.0)])
        at = rng.permutation(n)[:min(n, len(sp))]
        x[at] = sp[:len(at)]
    return x.astype(dtype)


def rows_input(n, xp_rows, seed, dtype=np.float64, specials=True):
    return np.stack([input_row(n, np.asarray(xp, dtype=np.float64), seed + 17 * r, dtype, specials)
                     for r, xp in enumerate(xp_rows)])


def gains_offsets(y, bits, seed):
    """per row of the referee's y: a gain whose sign alternates from row to row and which puts the rails' rounding
    boundaries at the row's 10th and 90th percentile (a curve's output is far from Gaussian: iir_dac_ref's 1.2 standard
    deviations need not be reached on both sides; a row of a few samples: iir_dac_ref's rule), and an offset that
    centres them plus a fraction of an LSB -- so that every row clips on both rails"""
    y = np.asarray(y, dtype=np.float64)
    if y.shape[1] < 64:
        return iref.gains_offsets(y, bits, seed)
    rng = np.random.default_rng(seed)
    half = 2.0**(bits - 1)
    q10, q90 = np.quantile(y, 0.1, axis=1), np.quantile(y, 0.9, axis=1)
    gain = half / np.maximum(0.5 * (q90 - q10), 1e-3) * np.where(np.arange(len(y)) % 2 == 0, 1.0, -1.0)
    offset = -gain * 0.5 * (q10 + q90) - 0.5 + rng.uniform(-0.45, 0.45, len(y))
    return gain, offset


class Case:
    """one batch: curves, ends, cascades, zi, levels, a gain / offset per row for `bits`, and two inputs -- `x`, finite
    (some samples beyond both ends of the knots, none NaN: the IIR-sensitive tests), and `x_special`, with the curve's
    specials (exact knots, end knots, just outside, NaN, +-Inf).  The referee's v (the curve's output), y, zf, codes,
    counts and beyond belong to `x`; `reference(x_special)` computes them for the other."""

    def __init__(self, nsec, order, batch, n, bits=16, shift=0, seed=None, dtype=np.float64, ends='default', first=None):
        self.nsec, self.order, self.batch, self.n, self.bits, self.shift = nsec, order, batch, n, bits, shift
        self.seed = 1000 * nsec + 100 * order + 7 * batch + n % 97 if seed is None else seed
        self.dtype = np.dtype(dtype)
        rng = np.random.default_rng(self.seed)
        self.xp, self.fp = curves_for(batch, self.seed % 7 if first is None else first)
        self.left, self.right = ends_for(batch, ends)
        self.rows = iref.random_rows(rng, batch, nsec, order)
        self.x = rows_input(n, self.xp, self.seed + 3, dtype, specials=False)
        self.x_special = rows_input(n, self.xp, self.seed + 3, dtype, specials=True)
        self.zi = rng.standard_normal((batch, nsec * order)) * 0.2
        self.initial = np.round(rng.uniform(-0.2, 0.2, batch), 3)
        self.v, self.y, self.zf = self.filtered(self.x)
        finite = np.where(np.isfinite(self.y), self.y, 0.0)
        self.gain, self.offset = gains_offsets(finite, bits, self.seed + 1)

    def filtered(self, x):
        """-> (v: the curve's output in the case's dtype, y: the cascades' output on it in float64, zf)"""
        v = cref.curve_ref(x, self.xp, self.fp, self.left, self.right)
        with np.errstate(invalid='ignore'):
            both = [iref.cascade(self.rows[r], v[r].astype(np.float64), self.zi[r], self.initial[r])
                    for r in range(self.batch)]
        return v, np.stack([b[0] for b in both]), np.stack([b[1] for b in both])

    def reference(self, x=None):
        """-> (codes, counts, beyond, zf) of the referee for `x` (None: the case's finite input)"""
        if x is None:
            y, zf, x = self.y, self.zf, self.x
        else:
            _, y, zf = self.filtered(x)
        codes, counts = dac_rows_ref.dac_ref(y, self.gain, self.offset, self.bits, self.shift)
        return codes, counts, cref.counts_ref(x, self.xp), zf

    def iir_case(self):
        """the IIR and converter part as an iir_dac_ref.Case on the curve's output: its tol_y and undecided"""
        c = iref.Case.__new__(iref.Case)
        c.nsec, c.order, c.batch, c.n, c.bits, c.shift = self.nsec, self.order, self.batch, self.n, self.bits, self.shift
        c.rows, c.x, c.zi, c.initial = self.rows, self.v.astype(np.float64), self.zi, self.initial
        c.y, c.zf, c.gain, c.offset = self.y, self.zf, self.gain, self.offset
        return c

    def tol_y(self):
        return self.iir_case().tol_y()

    def undecided(self, tol_y=None):
        return self.iir_case().undecided(tol_y)


# The cap on the undecided share is a CONDITION of the comparison with the referee, not a property of the device code:
# the first seeds from a case's default on for which every row stays at or below half of it (found from the referee alone)
REFEREE_SEEDS = {(1, 1): 1144, (1, 2): 1246, (1, 3): 1344, (1, 4): 1448, (2, 1): 2145, (3, 1): 3145, (4, 1): 4144,
                 (2, 2): 2244}


def referee_cases():
    """the batches the GPU test holds against the referee (float64, finite inputs; the undecided share of each, from the
    referee alone, is held to MAX_UNDECIDED_SHARE by tests/test_curve_iir_dac_cpu.py): every shape over two tiles and a
    sample on three curves of the pool (the row whose range overflows is left to the bit-for-bit tests), and the order-3
    section over two tiles and a part in the two narrower formats"""
    out = [Case(nsec, order, 3, TILE + 1, first=i % 4, seed=REFEREE_SEEDS[nsec, order])
           for i, (nsec, order) in enumerate(SHAPES)]
    out += [Case(1, 3, 3, 12000, bits, shift, first=1, seed=1390) for bits, shift in FORMATS[1:]]
    return out
