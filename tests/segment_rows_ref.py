"""Referee of the segment stage (distortion.SegmentStage / segment_rows, csrc/wfk_segment_rows.hip): the semantics in
NumPy, twice -- a plain double loop that restates the definition word for word and a vectorised form on np.diff /
np.flatnonzero / np.cumsum -- and the builders of the masks the tests use.

Per row g of n samples of k = width int16 codes, granules of A = align samples, Q = ceil(n / A):
    m[g, i]  = any_j ((codes[g, i k + j] >> bit) & 1)        (bit form)      or      marks[g, i] != 0   (marks form)
    G[g, q]  = any m[g, i] for i in [q A, min((q + 1) A, n))
    segments = the maximal runs [q0, q1) of G = 1, ascending:
               start = q0 A, length = min(q1 A, n) - start, offset = the lengths before it; kept = all lengths
    table    = [[start, length, offset], ...] int32,  packed = the k codes of every kept sample, in order
Everything is an integer: every comparison against this file is exact."""
import numpy as np


def mask_of(codes, width=1, bit=None, marks=None):
    """-> bool (rows, n): the mask of either form"""
    codes = np.asarray(codes)
    assert codes.dtype == np.int16 and codes.ndim == 2 and codes.shape[1] % width == 0
    assert (bit is None) != (marks is None)
    rows, n = codes.shape[0], codes.shape[1] // width
    if marks is not None:
        marks = np.asarray(marks)
        assert marks.shape == (rows, n)
        return marks != 0
    assert 0 <= bit <= 15
    bits = (codes.view(np.uint16) >> np.uint16(bit)) & np.uint16(1)
    return bits.reshape(rows, n, width).any(axis=2)


def segments_loop(m, align):
    """one row's mask (n,) -> [[start, length, offset], ...] by the definition: a loop over the granules in a loop
    over the samples of each"""
    n = len(m)
    table, run_start, offset = [], None, 0
    granules = -(-n // align)
    for q in range(granules + 1):
        on = False
        if q < granules:
            for i in range(q * align, min((q + 1) * align, n)):
                if m[i]:
                    on = True
                    break
        if on and run_start is None:
            run_start = q * align
        if not on and run_start is not None:
            length = min(q * align, n) - run_start
            table.append([run_start, length, offset])
            offset += length
            run_start = None
    return table


def segments_vector(m, align):
    """the same through np.diff of the granule bits, np.flatnonzero and np.cumsum"""
    m = np.asarray(m, dtype=bool)
    n = len(m)
    granules = -(-n // align)
    padded = np.zeros(granules * align, dtype=bool)
    padded[:n] = m
    g = padded.reshape(granules, align).any(axis=1) if granules else np.zeros(0, dtype=bool)
    edges = np.diff(np.concatenate([[0], g.astype(np.int8), [0]]))
    q0, q1 = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
    start = q0 * align
    length = np.minimum(q1 * align, n) - start
    offset = np.cumsum(length) - length
    return np.stack([start, length, offset], axis=1).tolist() if len(q0) else []


def segment_ref(codes, width=1, align=1, bit=None, marks=None, form='vector'):
    """-> (tables: a list per row of (count, 3) int32, packed: a list per row of (width * kept,) int16,
    used int64 (rows, 2) [count, kept])"""
    codes = np.asarray(codes)
    m = mask_of(codes, width, bit, marks)
    cut = segments_vector if form == 'vector' else segments_loop
    tables, packed, used = [], [], np.zeros((codes.shape[0], 2), dtype=np.int64)
    for g in range(codes.shape[0]):
        t = np.asarray(cut(m[g], align), dtype=np.int32).reshape(-1, 3)
        pieces = [codes[g, width * s:width * (s + l)] for s, l, _ in t.tolist()]
        tables.append(t)
        packed.append(np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int16))
        used[g] = [len(t), int(t[:, 1].sum())]
    return tables, packed, used


# ---- masks ----------------------------------------------------------------------------------------------------------

def bursts_mask(rows, n, seed, duty=0.2, gate=40):
    """random bursts of 1 .. 2 gate samples at about `duty`"""
    rng = np.random.default_rng(seed)
    m = np.zeros((rows, n), dtype=bool)
    gap = max(int(gate / duty - gate), 1)
    for r in range(rows):
        i = int(rng.integers(0, gap + 1))
        while i < n:
            length = int(rng.integers(1, 2 * gate + 1))
            m[r, i:i + length] = True
            i += length + int(rng.integers(1, 2 * gap + 1))
    return m


def alternate_mask(rows, n, align, phase=0):
    """every other granule on (its first sample, which every granule of a row has): the most segments a row can have"""
    m = np.zeros((rows, n), dtype=bool)
    i = np.arange(n)
    m[:, ((i // align) % 2 == phase) & (i % align == 0)] = True
    return m


def codes_with(m, width, bit, seed, one_code_only=False):
    """random int16 codes (rows, width n) whose bit `bit` is the mask (on every code of a sample, or -- `one_code_only`
    -- on a random one of its k codes); every other bit is in use"""
    m = np.asarray(m, dtype=bool)
    rows, n = m.shape
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 65536, (rows, n, width)).astype(np.uint16) & ~np.uint16(1 << bit)
    which = np.ones((rows, n, width), dtype=bool)
    if one_code_only and width == 2:
        first = rng.integers(0, 2, (rows, n)).astype(bool)
        which = np.stack([first, ~first], axis=2)
    u |= ((m[:, :, None] & which).astype(np.uint16) << np.uint16(bit))
    return u.reshape(rows, n * width).view(np.int16)
