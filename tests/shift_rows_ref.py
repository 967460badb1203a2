"""Referee of the per-row shift (distortion.ShiftStage / shift_rows): the closed form of the reference's
shift(signal, delay, dt), written from its definition in vectorised NumPy.

    p = int(delay // dt),   d = delay / dt - p                       (Python floats; d in [0, 1])
    s[j] = (1 - d) x[j] + d x[j - 1]   if d > 0   (x[-1] = 0),      s[j] = x[j] otherwise
    y[i] = s[i - p]   if 0 <= i - p < n,   0 otherwise

Next to y it gives B, the scale of an element's rounding error: B[i] = |1 - d| |x[i - p]| + |d| |x[i - p - 1]| where
y[i] comes from samples, 0 where it is zero fill.  Two implementations of the form that each round two products and
one sum (relative 2^-53 apiece, the sum's on a value of at most B) differ by at most 2 * 2 * 2^-53 * B: BOUND.
"""
import numpy as np

BOUND = 4 * 2.0**-53          # times B: per element, float64 rows
EPS32 = 2.0**-24              # float32 rows: one more rounding, of the result itself


def split(delay, dt):
    """(p, d) with the reference's own expressions"""
    p = int(delay // dt)
    return p, delay / dt - p


def shift_ref(x, p, d):
    """one row -> (y, B), both float64 arrays of len(x); x is taken as float64"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    y, B = np.zeros(n), np.zeros(n)
    i = np.arange(n)
    j = i - p
    ok = (j >= 0) & (j < n)
    jj = j[ok]
    cur = x[jj]
    if d > 0:
        prev = np.where(jj >= 1, x[np.maximum(jj - 1, 0)], 0.0)
        with np.errstate(invalid='ignore', over='ignore'):
            y[ok] = (1 - d) * cur + d * prev
            B[ok] = abs(1 - d) * np.abs(cur) + abs(d) * np.abs(prev)
    else:
        y[ok] = cur
        B[ok] = np.abs(cur)
    return y, B


def shift_rows_ref(x, points, deltas):
    """rows -> (y, B) of x's shape"""
    ys, Bs = zip(*[shift_ref(row, p, d) for row, p, d in zip(x, points, deltas)])
    return np.stack(ys), np.stack(Bs)


def check(got, want, B, what='', eps_out=0.0):
    """|got - want| <= BOUND * B + eps_out * |want| per element, and exactly 0 where B = 0; prints the worst ratio"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.abs(got - want)
    tol = BOUND * B + eps_out * np.abs(want)
    zero = B == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(tol > 0, diff / tol, 0.0)
    print(f'{what}: worst |diff| / bound = {float(ratio.max()) if ratio.size else 0.0:.3g}')
    assert np.all(got[zero] == 0.0), f'{what}: a zero-fill element is not zero'
    assert np.all(diff <= tol), f'{what}: worst |diff| / bound = {float(ratio.max()):.3g}'
