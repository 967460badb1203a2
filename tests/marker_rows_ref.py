"""Referee of the marker stage (distortion.MarkerStage / marker_rows, csrc/wfk_marker_rows.hip): the semantics in
NumPy, twice -- a brute-force double loop that restates the definition word for word (rows of up to 300 samples) and
a cumulative-sum form for rows of any length -- and the builder of the input rows the tests use.

Per marker row g of k = group input rows:
    active[g, i] = any_j  fabs(float64(x[g k + j, i])) > threshold[g]       (NaN inactive, +-inf active)
    m[g, i]      = any    active[g, j]  for j in [i - trail[g], i + lead[g]], clipped to [0, n)
    counts[g]    = [high, pulses]: the i with m = 1, and those of them with i = 0 or m[g, i - 1] = 0
Markers and counts are integers: every comparison against this file is exact."""
import numpy as np

BRUTE_MAX = 300
KINDS = ('spikes', 'bursts', 'zero', 'active', 'specials')


def _per_row(v, rows, dtype):
    return np.broadcast_to(np.asarray(v, dtype=dtype), (rows,))


def active_rows(x, threshold, group=1):
    """x (batch, n) -> bool (batch // group, n)"""
    x = np.asarray(x)
    batch, n = x.shape
    assert batch % group == 0
    rows = batch // group
    thr = _per_row(threshold, rows, np.float64)
    with np.errstate(all='ignore'):
        a = np.abs(x.astype(np.float64)).reshape(rows, group, n) > thr[:, None, None]
    return a.any(axis=1)


def counts_of(m):
    """m (rows, n) 0 / 1 -> int64 (rows, 2) [high, pulses]"""
    m = np.asarray(m).astype(bool)
    before = np.zeros_like(m)
    before[:, 1:] = m[:, :-1]
    return np.stack([m.sum(axis=1), (m & ~before).sum(axis=1)], axis=1).astype(np.int64)


def marker_brute(x, lead, trail, threshold=0.0, group=1):
    """the definition as a double loop; rows of at most BRUTE_MAX samples"""
    a = active_rows(x, threshold, group)
    rows, n = a.shape
    assert n <= BRUTE_MAX
    lead, trail = _per_row(lead, rows, np.int64), _per_row(trail, rows, np.int64)
    m = np.zeros((rows, n), dtype=np.uint8)
    for g in range(rows):
        for i in range(n):
            for j in range(i - int(trail[g]), i + int(lead[g]) + 1):
                if 0 <= j < n and a[g, j]:
                    m[g, i] = 1
                    break
    return m, counts_of(m)


def marker_cumsum(x, lead, trail, threshold=0.0, group=1):
    """the same through a running count of the active samples: m[i] = S[min(i + lead, n - 1) + 1] > S[max(i - trail, 0)]"""
    a = active_rows(x, threshold, group)
    rows, n = a.shape
    lead, trail = _per_row(lead, rows, np.int64), _per_row(trail, rows, np.int64)
    m = np.zeros((rows, n), dtype=np.uint8)
    i = np.arange(n, dtype=np.int64)
    for g in range(rows):
        s = np.concatenate([[0], np.cumsum(a[g], dtype=np.int64)])
        hi = np.minimum(i + lead[g], n - 1) + 1
        lo = np.maximum(i - trail[g], 0)
        m[g] = s[hi] > s[lo] if n else 0
    return m, counts_of(m)


def marker_ref(x, lead, trail, threshold=0.0, group=1):
    """x (batch, n) float64 / float32 -> (m uint8 (batch // group, n), counts int64 (batch // group, 2))"""
    return marker_cumsum(x, lead, trail, threshold, group)


def into_codes(codes, m, group=1, bit=0):
    """codes int16 (rows, group n), m (rows, n) -> a copy with codes[g, p] = (codes[g, p] & ~(1 << bit)) |
    (m[g, p // group] << bit)"""
    codes = np.asarray(codes)
    assert codes.dtype == np.int16 and codes.shape == (m.shape[0], group * m.shape[1]) and 0 <= bit <= 15
    u = codes.view(np.uint16).astype(np.uint32)
    mm = np.repeat(np.asarray(m).astype(np.uint32), group, axis=1)
    return ((u & ~np.uint32(1 << bit) & 0xffff) | (mm << bit)).astype(np.uint16).view(np.int16)


def specials(threshold, dtype=np.float64):
    """the values the definition treats one by one, and their negatives -> (values, active) in `dtype`: NaN, inf,
    0.0 (-0.0 with it), a subnormal, the threshold itself (as `dtype` holds it) and the next value above it"""
    dt = np.dtype(dtype).type
    t = dt(threshold)
    vals = np.array([np.nan, np.inf, 0.0, np.finfo(dt).smallest_subnormal, t, np.nextafter(t, dt(np.inf))], dtype=dt)
    vals = np.concatenate([vals, -vals])
    with np.errstate(all='ignore'):
        return vals, np.abs(vals.astype(np.float64)) > np.float64(threshold)


def rows_pattern(rows, n, seed, kind, dtype=np.float64, threshold=0.0, positions=None, burst=40, gap=300):
    """(rows, n) input rows of `dtype`, exact zeros where they are not active.
    'spikes': single samples at `positions` (one list for every row, or a list per row);  'bursts': runs of 1 .. burst
    samples above the threshold, of both signs, with gaps of 1 .. gap zeros (and small values below a non-zero
    threshold in the gaps);  'zero' / 'active': nothing / everything above the threshold;  'specials': `specials()`
    scattered over rows that are otherwise zero, the rest of a short row cut off."""
    assert kind in KINDS
    rng = np.random.default_rng(seed)
    x = np.zeros((rows, n), dtype=np.float64)
    big = 2.0 * threshold + 1.0
    if kind == 'spikes':
        per_row = positions if positions and np.ndim(positions[0]) > 0 else [positions or []] * rows
        for r in range(rows):
            for p in per_row[r]:
                if 0 <= p < n:
                    x[r, p] = big if (p + r) % 2 else -big
    elif kind == 'bursts':
        for r in range(rows):
            i = int(rng.integers(0, gap + 1))
            while i < n:
                length = int(rng.integers(1, burst + 1))
                x[r, i:i + length] = rng.uniform(big, 2 * big, min(length, n - i)) * rng.choice([-1.0, 1.0])
                i += length + int(rng.integers(1, gap + 1))
        if threshold > 0:
            quiet = x == 0
            x[quiet] = rng.uniform(-0.9 * threshold, 0.9 * threshold, int(quiet.sum()))
    elif kind == 'active':
        x[:] = rng.uniform(big, 2 * big, (rows, n)) * rng.choice([-1.0, 1.0], (rows, n))
    x = x.astype(dtype)
    if kind == 'specials':
        vals, _ = specials(threshold, dtype)
        for r in range(rows):
            at = rng.permutation(n)[:len(vals)] if n >= len(vals) else np.arange(n)
            x[r, at] = rng.permutation(vals)[:len(at)]
    return x
