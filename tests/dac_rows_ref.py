"""Referee of the DAC stage (distortion.DacStage / dac_codes_rows, csrc/wfk_dac_rows.hip): the semantics in NumPy, and
the builder of rows on which a fused multiply-add or another rounding mode gives other codes.

Per input row r, in float64 (a float32 sample is widened first; NumPy rounds the product, then the sum):
    v = x[r] * gain[r] + offset[r];  q = rint(v), half to even;  lo = -2**(bits - 1), hi = 2**(bits - 1) - 1
    c = 0 where v is NaN (nan), lo where q < lo (below), hi where q > hi (above), q otherwise
    word = c * 2**shift as int16;  out[g, i k + j] = word[g k + j, i] for interleave k
Codes and counts are integers: every comparison against this file is exact."""
from fractions import Fraction

import numpy as np


def rails(bits):
    return -2**(bits - 1), 2**(bits - 1) - 1


def dac_ref(x, gain, offset=0.0, bits=16, shift=0, interleave=1):
    """x (batch, n) float64 / float32 -> (codes int16 (batch // k, k n), counts int64 (batch, 3) [below, above, nan])"""
    x = np.asarray(x)
    batch, n = x.shape
    g = np.broadcast_to(np.asarray(gain, dtype=np.float64), (batch,))
    o = np.broadcast_to(np.asarray(offset, dtype=np.float64), (batch,))
    lo, hi = rails(bits)
    k = interleave
    assert batch % k == 0 and 2 <= bits <= 16 and 0 <= shift <= 16 - bits
    with np.errstate(all='ignore'):
        v = x.astype(np.float64) * g[:, None] + o[:, None]
        q = np.rint(v)
        nan, below, above = np.isnan(v), q < lo, q > hi
        c = np.where(nan, 0.0, np.where(below, lo, np.where(above, hi, q)))
    word = (c.astype(np.int64) * 2**shift).astype(np.int16)
    codes = word.reshape(batch // k, k, n).transpose(0, 2, 1).reshape(batch // k, k * n)
    counts = np.stack([below.sum(axis=1), above.sum(axis=1), nan.sum(axis=1)], axis=1).astype(np.int64)
    return np.ascontiguousarray(codes), counts


def sensitive_row(count=1024, g=9731.37, M=20000, seed=7, span=600, ulps=4):
    """-> (x float64 (count,), ks int64 (count,)): samples with fl(x[i] * g) == M + ks[i] + 0.5 EXACTLY, so that with
    gain g and offset -M the two-rounding result v is the exact tie ks[i] + 0.5, while the fused fl(x g - M) keeps the
    product's rounding error and falls off the tie.  Found by stepping x a few ulps around (M + k + 0.5) / g; a k for
    which no neighbour's product rounds onto the tie is skipped."""
    rng = np.random.default_rng(seed)
    xs, ks = [], []
    while len(xs) < count:
        k = int(rng.integers(-span, span))
        t = M + k + 0.5
        x = t / g
        cands = [x]
        up = dn = x
        for _ in range(ulps):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            cands += [up, dn]
        hit = [c for c in cands if float(c) * g == t]
        if hit:
            xs.append(float(hit[0]))
            ks.append(k)
    return np.array(xs, dtype=np.float64), np.array(ks, dtype=np.int64)


def fused_value(x, g, M):
    """fl(x g - M): ONE rounding of the exact value"""
    return float(Fraction(float(x)) * Fraction(float(g)) - M)


def half_away(v):
    """round half away from zero"""
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def tie_row32(count=1024, seed=11, span=2000, log2_gain=10):
    """-> (x float32 (count,), ks, gain): x[i] = (ks[i] + 0.5) / gain with gain = 2**log2_gain, exact in float32, so
    that x gain + (an integer offset) is an exact tie: float32 rows test the rounding mode (a 24-bit sample cannot be
    steered onto a tie through a 53-bit gain)"""
    rng = np.random.default_rng(seed)
    ks = rng.integers(-span, span, count).astype(np.int64)
    gain = float(2**log2_gain)
    x = ((ks + 0.5) / gain).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * gain, ks + 0.5)
    return x, ks, gain
