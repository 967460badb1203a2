"""Referee of the fused mix-to-codes stage (distortion.MixDacStage / mix_dac_rows, csrc/wfk_mix_dac.hip): the two
referees it is made of, one after the other, and the builder of rows on which the MIX half's order of summation or a
fused multiply-add shows in the CODES -- the only place where the fused stage lets the mixed row be seen.

    codes, counts = dac_ref(mix_ref(x, matrix, mix_offset), gain, dac_offset, bits, shift, interleave)
Codes and counts are integers: every comparison against this file is exact."""
from fractions import Fraction

import numpy as np

import dac_rows_ref
import mix_rows_ref

TIE_GAIN = 2.0**42                 # one ulp of a mixed value in [512, 1024), 2**-43, is half an LSB
TIE_CENTRE = 768.0
TIE_OFFSET = -TIE_CENTRE * TIE_GAIN


def mix_dac_ref(x, matrix, mix_offset, gain, dac_offset=0.0, bits=16, shift=0, interleave=1):
    """x (rows_in, n) float64 / float32 -> (codes int16 (rows_out // k, k n), counts int64 (rows_out, 3))"""
    return dac_rows_ref.dac_ref(mix_rows_ref.mix_ref(x, matrix, mix_offset), gain, dac_offset, bits, shift, interleave)


def tie_code(y):
    """the 16-bit code of the mixed value y under TIE_GAIN / TIE_OFFSET (exact: both steps are)"""
    return int(dac_rows_ref.dac_ref(np.array([[y]], dtype=np.float64), TIE_GAIN, TIE_OFFSET)[0][0, 0])


def descending(x, m):
    return mix_rows_ref.ascending(x[::-1], m[::-1])


def tie_case(count=256, seed=5):
    """-> (x float64 (3, count), m float64 (1, 3)): mix_rows_ref.sensitive_case's row, its samples steered so that the
    ascending two-rounding sum y lies within 2**-28 of 768.  With gain TIE_GAIN and offset TIE_OFFSET the converter's
    v = (y - 768) * 2**42 is EXACT and a multiple of 0.5 LSB, so a y that is one ulp off gives another v, and a sample
    is kept only where that shows: the code of the ascending sum differs from the code of the descending sum AND from
    the code of the sum whose every step is a fused multiply-add, and lies inside +-32000 (no clipping).  Held again,
    in exact rational arithmetic, by tests/test_mix_dac_cpu.py."""
    rng = np.random.default_rng(seed)
    m = np.array([[0.7310585786300049, -1.9130434782608696e3, 3.141592653589793e-3]])
    cols = []
    while len(cols) < count:
        x0, x1 = rng.uniform(-1e3, 1e3), rng.uniform(-1.0, 1.0)
        target = TIE_CENTRE + float(rng.integers(-63000, 63001)) * 2.0**-43
        x2 = (target - (x0 * m[0, 0] + x1 * m[0, 1])) / m[0, 2]
        x = np.array([x0, x1, x2])
        y = mix_rows_ref.ascending(x, m[0])
        if abs(y - TIE_CENTRE) > 2.0**-28:
            continue
        code = tie_code(y)
        if abs(code) <= 32000 and code != tie_code(descending(x, m[0])) and code != tie_code(mix_rows_ref.fused(x, m[0])):
            cols.append(x)
    return np.ascontiguousarray(np.array(cols).T), m


def exact_v(y):
    """(y - 768) * 2**42 as a Fraction: what the converter's two roundings give exactly for y near 768"""
    return (Fraction(float(y)) - Fraction(TIE_CENTRE)) * Fraction(TIE_GAIN)
