"""The referee of the curve stage (distortion.CurveStage / interp_rows, csrc/wfk_curve_rows.hip): its semantics in NumPy
element operations, every operation rounded on its own, next to the builders of the cases both test files use.  A plain
module like dac_rows_ref.py; nothing here touches a device.

Per row r with knots xp (finite, strictly increasing, K >= 2), values fp, slope[j] = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]):
    x is NaN -> x;   x < xp[0] -> left;   x > xp[K-1] -> right;
    j = searchsorted(xp, x, 'right') - 1;   x == xp[j] (j = K-1 is that case) -> fp[j];
    otherwise slope[j] * (x - xp[j]) + fp[j], the difference, the product and the sum each rounded to float64;
a float32 row is widened first and its result rounded once.  tests/test_curve_rows_cpu.py holds this to np.interp, bit for
bit."""
from fractions import Fraction

import numpy as np

MAX_KNOTS = 1024


def _rows(rows, batch):
    """a list of 1-D float64 arrays, one per row (one array: every row's)"""
    if isinstance(rows, np.ndarray) and rows.ndim == 1 or np.ndim(rows[0]) == 0:
        return [np.asarray(rows, dtype=np.float64)] * batch
    assert len(rows) == batch, (len(rows), batch)
    return [np.asarray(r, dtype=np.float64) for r in rows]


def _ends(v, default, batch):
    if v is None:
        return np.array(default, dtype=np.float64)
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (batch, )).copy()


def curve_row(x, xp, fp, left, right):
    """one row; x float64 or float32 -> the same dtype"""
    x64 = np.asarray(x).astype(np.float64)
    slope = (fp[1:] - fp[:-1]) / (xp[1:] - xp[:-1])                  # each operation an array operation: rounded on its own
    slope = np.append(slope, 0.0)
    nan, below, above = np.isnan(x64), x64 < xp[0], x64 > xp[-1]
    xs = np.where(nan | below | above, xp[0], x64)
    j = np.searchsorted(xp, xs, 'right') - 1
    d = xs - xp[j]
    p = slope[j] * d
    y = p + fp[j]
    y = np.where(xs == xp[j], fp[j], y)
    y = np.where(below, left, np.where(above, right, y))
    y = np.where(nan, x64, y)
    return y.astype(np.asarray(x).dtype)


def curve_ref(x, xp_rows, fp_rows, left=None, right=None):
    """x (rows, n) float64 / float32 -> the stage's output, the same shape and dtype"""
    x = np.asarray(x)
    batch = x.shape[0]
    xs, fs = _rows(xp_rows, batch), _rows(fp_rows, batch)
    left, right = _ends(left, [f[0] for f in fs], batch), _ends(right, [f[-1] for f in fs], batch)
    return np.stack([curve_row(x[r], xs[r], fs[r], left[r], right[r]) for r in range(batch)])


def counts_ref(x, xp_rows):
    """(rows, 3) int64 [below, above, nan] per row"""
    x = np.asarray(x).astype(np.float64)
    xs = _rows(xp_rows, x.shape[0])
    return np.array([[np.count_nonzero(x[r] < xs[r][0]), np.count_nonzero(x[r] > xs[r][-1]),
                      np.count_nonzero(np.isnan(x[r]))] for r in range(x.shape[0])], dtype=np.int64)


def same_bits(got, want, what):
    """bits equal wherever the referee is not NaN, and NaN exactly where the referee has NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    raw = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), np.ascontiguousarray(got).view(raw) != np.ascontiguousarray(want).view(raw))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {np.count_nonzero(bad)} of {bad.size} differ, first at {at}: got {got[at]!r}, '
                             f'want {want[at]!r}')


# ---- knot sets ----------------------------------------------------------------------------------------------------------
def uniform_knots(K, lo=-1.0, hi=1.0, seed=0):
    """K evenly spaced knots over [lo, hi] and a monotone, visibly non-linear curve over them"""
    xp = np.linspace(lo, hi, K)
    rng = np.random.default_rng(1000 + K + seed)
    fp = np.cumsum(rng.uniform(0.1, 1.0, K)) * (0.7 / K) - 0.31
    return xp, fp


def log_knots(K, lo=1e-4, hi=1.0, seed=0):
    """K log-spaced knots over [lo, hi] (dense at the low end: many knots in one bucket of a uniform table) and a curve
    that is not monotone"""
    xp = np.geomspace(lo, hi, K)
    assert np.all(np.diff(xp) > 0)
    rng = np.random.default_rng(2000 + K + seed)
    fp = np.sin(np.linspace(0.0, 9.0, K)) * 0.4 + rng.uniform(-0.01, 0.01, K)
    return xp, fp


def knots(K, spacing, seed=0):
    return (uniform_knots if spacing == 'uniform' else log_knots)(K, seed=seed)


def ragged_batch():
    """three rows: 2 knots, 1024 log-spaced knots, 65 uniform knots"""
    a = (np.array([-0.5, 0.75]), np.array([2.0, -3.0]))
    pairs = [a, log_knots(1024), uniform_knots(65)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def knot_edges(xp):
    """every knot and its two neighbours by nextafter: 3 K values"""
    return np.concatenate([xp, np.nextafter(xp, -np.inf), np.nextafter(xp, np.inf)])


def row_input(n, xp, seed, dtype=np.float64, specials=True):
    """n samples for a row with knots xp: mostly inside [xp[0], xp[-1]], some beyond both ends, and -- `specials`, as
    far as n allows, scattered over the row -- every knot, nextafter on both sides of knots, +-inf, NaN, +-0.0"""
    rng = np.random.default_rng(seed)
    w = xp[-1] - xp[0]
    x = rng.uniform(xp[0] - 0.05 * w, xp[-1] + 0.05 * w, n)
    if specials and n:
        sp = np.concatenate([[np.nan, np.inf, -np.inf, 0.0, -0.0, xp[0], xp[-1]], knot_edges(xp)])
        at = rng.permutation(n)[:min(n, len(sp))]
        x[at] = rng.permutation(sp)[:len(at)] if len(at) < len(sp) else sp
        if n >= 7:
            x[at[:7]] = sp[:7]
    return x.astype(dtype)


def rows_input(n, xp_rows, seed, dtype=np.float64, specials=True):
    return np.stack([row_input(n, np.asarray(xp, dtype=np.float64), seed + 17 * r, dtype, specials)
                     for r, xp in enumerate(xp_rows)])


# ---- the contraction-sensitive case ---------------------------------------------------------------------------------------
def sensitive_case(n=4096, K=33, seed=5):
    """knots, values and samples with full 53-bit mantissas everywhere, the values a zigzag through zero: the product
    slope * (x - xp[j]) is inexact on almost every sample and mostly cancels against fp[j], so its rounding error is
    above the last bit of the sum, and an evaluation that adds fp[j] to the EXACT product (a fused multiply-add) rounds
    differently on about half of the samples.  -> (x (1, n), xp, fp)"""
    rng = np.random.default_rng(seed)
    xp = np.cumsum(rng.uniform(0.5, 1.5, K))
    fp = rng.uniform(0.5, 1.5, K) * np.where(np.arange(K) % 2, -1.0, 1.0)
    x = rng.uniform(xp[0], xp[-1], (1, n))
    return x, xp, fp


def fused_row(x, xp, fp):
    """the row with the last two operations fused, in exact rational arithmetic: fl(slope[j] * d + fp[j]), d = fl(x -
    xp[j]), for samples inside the knots that hit none of them"""
    slope = (fp[1:] - fp[:-1]) / (xp[1:] - xp[:-1])
    j = np.searchsorted(xp, x, 'right') - 1
    assert np.all((j >= 0) & (j < len(xp) - 1) & (x != xp[j]))
    d = x - xp[j]
    return np.array([float(Fraction(float(slope[k])) * Fraction(float(dd)) + Fraction(float(fp[k])))
                     for k, dd in zip(j, d)])
