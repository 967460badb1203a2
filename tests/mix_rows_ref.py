"""Referee of the mix stage (distortion.MixStage / mix_rows, csrc/wfk_mix_rows.hip): the semantics as a plain NumPy loop
over terms, and the builders of the matrices and rows its tests use.

A term of output row o is an entry M[o, c] != 0.  Per sample, in float64 (a float32 sample is widened first; NumPy
rounds the product, then the sum), terms in ascending c:
    acc = 0.0;   acc = acc + x[c] * M[o, c]   for every term;   y[o] = acc + offset[o]
and a float32 result is rounded once, by `.astype(np.float32)`.  An input row on which o has no term is not read for
o.  The kernel does the same arithmetic in the same order: every comparison against this file is exact."""
from fractions import Fraction

import numpy as np


def mix_ref(x, matrix, offset=None):
    """x (rows_in, n) float64 / float32, matrix (rows_out, rows_in) -> y (rows_out, n) of x's dtype"""
    x = np.asarray(x)
    m = np.asarray(matrix, dtype=np.float64)
    assert x.ndim == 2 and m.ndim == 2 and m.shape[1] == x.shape[0] and x.dtype in (np.float64, np.float32)
    off = np.zeros(m.shape[0]) if offset is None else np.broadcast_to(np.asarray(offset, dtype=np.float64), (m.shape[0],))
    y = np.empty((m.shape[0], x.shape[1]), dtype=x.dtype)
    with np.errstate(all='ignore'):
        for o in range(m.shape[0]):
            acc = np.zeros(x.shape[1], dtype=np.float64)
            for c in np.flatnonzero(m[o]):                   # ascending
                acc = acc + x[c].astype(np.float64) * m[o, c]
            y[o] = (acc + off[o]).astype(x.dtype)
    return y


def same_bits(got, want, what):
    """bits equal wherever `want` is not NaN, NaN exactly where `want` has NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    raw = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    bad = np.isnan(got) != nan
    bad |= ~nan & (np.ascontiguousarray(got).view(raw) != np.ascontiguousarray(want).view(raw))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} differ, first at {at}: got {got[at]!r}, want {want[at]!r}')


# ---- matrices --------------------------------------------------------------------------------------------------------
def iq_blocks(pairs, seed=0):
    """-> (blocks, offset): per pair a 2 x 2 matrix near the identity (gain imbalance, phase skew) and two DC offsets"""
    rng = np.random.default_rng(seed)
    blocks = [np.array([[1.0 + 0.05 * rng.standard_normal(), 0.08 * rng.standard_normal()],
                        [0.08 * rng.standard_normal(), 1.0 + 0.05 * rng.standard_normal()]]) for _ in range(pairs)]
    return blocks, 0.01 * rng.standard_normal(2 * pairs)


def block_diagonal(blocks):
    blocks = [np.asarray(b, dtype=np.float64) for b in blocks]
    m = np.zeros((sum(b.shape[0] for b in blocks), sum(b.shape[1] for b in blocks)))
    r = c = 0
    for b in blocks:
        m[r:r + b.shape[0], c:c + b.shape[1]] = b
        r, c = r + b.shape[0], c + b.shape[1]
    return m


def band(rows, half_width, seed=0):
    """rows x rows, 1 + small on the diagonal, small non-zero entries up to `half_width` off it"""
    rng = np.random.default_rng(seed)
    m = np.zeros((rows, rows))
    for o in range(rows):
        for c in range(max(0, o - half_width), min(rows, o + half_width + 1)):
            m[o, c] = (1.0 if c == o else 0.0) + 0.03 * rng.uniform(0.2, 1.0) * rng.choice([-1.0, 1.0])
    return m


def dense(rows_out, rows_in, seed=0):
    """no zero anywhere"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 1.0, (rows_out, rows_in)) * rng.choice([-1.0, 1.0], (rows_out, rows_in))


def permutation(rows, seed=0):
    """-> (matrix, perm): y[o] = x[perm[o]]"""
    perm = np.random.default_rng(seed).permutation(rows)
    m = np.zeros((rows, rows))
    m[np.arange(rows), perm] = 1.0
    return m, perm


def one_long_row(rows, terms, long_row, seed=0):
    """rows x max(rows, terms): row `long_row` has `terms` terms (columns 0 .. terms - 1), every other row one term,
    on its own column"""
    rng = np.random.default_rng(seed)
    m = np.zeros((rows, max(rows, terms)))
    m[np.arange(rows), np.arange(rows)] = rng.uniform(0.5, 1.5, rows)
    m[long_row, :terms] = rng.uniform(0.1, 1.0, terms) * rng.choice([-1.0, 1.0], terms)
    return m


def reads_of(matrix, tile):
    """the sum over tiles of `tile` consecutive output rows of the number of columns the tile has a non-zero on"""
    m = np.asarray(matrix)
    return sum(int(np.count_nonzero(np.any(m[o:o + tile] != 0, axis=0))) for o in range(0, m.shape[0], tile))


# ---- rows ------------------------------------------------------------------------------------------------------------
def rows_input(rows, n, seed, dtype=np.float64, specials=True):
    """samples in [-1, 1] with +-inf, NaN and -0.0 scattered in them"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (rows, n))
    if specials:
        flat = x.reshape(-1)
        for start, step, v in ((0, 7, np.inf), (1, 11, -np.inf), (2, 13, np.nan), (3, 17, -0.0)):
            flat[start % flat.size::step * max(1, flat.size // 97)] = v
    return x.astype(dtype)


def sensitive_case(count=512, seed=3):
    """-> (x float64 (3, count), m float64 (1, 3)): one output row with three terms on which, for every sample,
      (a) the order matters: ((p0 + p1) + p2) in ascending c differs in its bits from ((p2 + p1) + p0), and
      (b) contraction matters: the sum of rounded products p_c = fl(x[c] m[c]) differs from the one whose every step
          is a fused fl(acc + x[c] m[c]).
    Found by drawing samples and keeping those that show both (held again by
    tests/test_mix_rows_cpu.py in exact rational arithmetic)."""
    rng = np.random.default_rng(seed)
    m = np.array([[0.7310585786300049, -1.9130434782608696e3, 3.141592653589793e-3]])
    cols = []
    while len(cols) < count:
        x = rng.uniform(-1.0, 1.0, 3) * np.array([1e3, 1.0, 1e2])
        if order_differs(x, m[0]) and fused_differs(x, m[0]):
            cols.append(x)
    return np.ascontiguousarray(np.array(cols).T), m


def ascending(x, m):
    acc = 0.0
    for xc, mc in zip(x, m):
        acc = acc + float(xc) * float(mc)
    return acc


def order_differs(x, m):
    return ascending(x, m) != ascending(x[::-1], m[::-1])


def fused(x, m):
    """the sum a fused multiply-add gives: every step fl(acc + x m) in ONE rounding of the exact value"""
    acc = 0.0
    for xc, mc in zip(x, m):
        acc = float(Fraction(acc) + Fraction(float(xc)) * Fraction(float(mc)))
    return acc


def fused_differs(x, m):
    return ascending(x, m) != fused(x, m)
