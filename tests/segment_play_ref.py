"""Referee of the segment player (distortion.SegmentPlayer / play_rows, csrc/wfk_segment_play.hip): the semantics in
NumPy, twice -- a loop over the segments, as distortion.expand_segments does it, and per sample through np.searchsorted
on the starts -- with the rule of the good rows, the report, and the builders of the inputs the tests use.

Per row of `count` entries [start, length, offset] over `packed` (k = width codes per sample), n samples:
    the row is GOOD when 0 <= count <= max_segments, every entry j < count has length > 0, start >= 0,
    start + length <= n, offset >= 0, offset + length <= capacity, and start_j >= start_(j-1) + length_(j-1) for
    1 <= j < count: ascending and disjoint (touching is good)
    out[i] = the k codes at k (offset_j + i - start_j) of packed where start_j <= i < start_j + length_j, else idle
    report = [played, differ, stray, first]: played = the lengths; with `expect`, differ = the samples inside a play
    where any of the k codes differs from expect, stray = the samples outside every play where any code of expect
    differs from its idle, first = the lowest sample counted by either or -1; without it [played, 0, 0, -1]
    a BAD row: report [-1, -1, -1, -1], nothing of out
This is NARROWER than expand_segments, which takes empty and overlapping entries (the later one wins); on a good row
the two agree bit for bit.  Everything is an integer: every comparison against this file is exact."""
import numpy as np


def idle_codes(idle, k):
    """one code or one per code of a sample -> k int16 codes"""
    idle = np.asarray(idle, dtype=np.int16).reshape(-1)
    assert len(idle) in (1, k)
    return np.resize(idle, k).astype(np.int16)


def row_is_good(table, count, n, max_segments, capacity):
    count = int(count)
    if count < 0 or count > max_segments:
        return False
    end = 0
    for j in range(count):
        start, length, offset = (int(v) for v in table[j])
        if length <= 0 or start < 0 or start + length > n or offset < 0 or offset + length > capacity or start < end:
            return False
        end = start + length
    return True


def play_row_loop(table, packed, count, n, idle, k):
    """one good row by a loop over its entries -> (out (k n,) int16, inside (n,) bool)"""
    out = np.tile(idle_codes(idle, k), n).astype(np.int16)
    inside = np.zeros(n, dtype=bool)
    for j in range(int(count)):
        start, length, offset = (int(v) for v in table[j])
        out[k * start:k * (start + length)] = packed[k * offset:k * (offset + length)]
        inside[start:start + length] = True
    return out, inside


def play_row_searchsorted(table, packed, count, n, idle, k):
    """the same per sample: the entry of sample i is the last one that starts at or before i"""
    count = int(count)
    t = np.asarray(table[:count], dtype=np.int64).reshape(-1, 3)
    i = np.arange(n, dtype=np.int64)
    j = np.searchsorted(t[:, 0], i, side='right') - 1
    jj = np.clip(j, 0, max(count - 1, 0))
    if count:
        inside = (j >= 0) & (i < t[jj, 0] + t[jj, 1])
        src = t[jj, 2] + i - t[jj, 0]
    else:
        inside, src = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    out = np.tile(idle_codes(idle, k), n).astype(np.int16).reshape(n, k)
    packed = np.asarray(packed)
    if inside.any():
        at = src[inside]
        out[inside] = np.stack([packed[k * at + q] for q in range(k)], axis=1)
    return out.reshape(-1), inside


def report_of(out, inside, expect, idle, k, played):
    """[played, differ, stray, first] of one good row"""
    if expect is None:
        return [played, 0, 0, -1]
    n = len(inside)
    d = (np.asarray(expect[:k * n]).reshape(n, k) != out.reshape(n, k)).any(axis=1)
    counted = np.flatnonzero(d)
    return [played, int((d & inside).sum()), int((d & ~inside).sum()), int(counted[0]) if len(counted) else -1]


def play_ref(table, packed, used, n, idle=0, k=1, capacity=None, expect=None, form='loop'):
    """table (rows, max_segments, 3) int32, packed (rows, >= k capacity) int16, used (rows, 2) int64, expect (rows,
    >= k n) int16 or None -> (out: a list per row, (k n,) int16 or None for a bad row, report (rows, 4) int64)"""
    table, packed, used = np.asarray(table), np.asarray(packed), np.asarray(used)
    rows, max_segments = table.shape[0], table.shape[1]
    capacity = packed.shape[1] // k if capacity is None else capacity
    one = play_row_loop if form == 'loop' else play_row_searchsorted
    outs, report = [], np.zeros((rows, 4), dtype=np.int64)
    for r in range(rows):
        count = int(used[r, 0])
        if not row_is_good(table[r], count, n, max_segments, capacity):
            outs.append(None)
            report[r] = -1
            continue
        out, inside = one(table[r], packed[r], count, n, idle, k)
        outs.append(out)
        played = int(np.asarray(table[r, :count, 1], dtype=np.int64).sum())
        report[r] = report_of(out, inside, None if expect is None else expect[r], idle_codes(idle, k), k, played)
    return outs, report


def expected_out(table, packed, used, n, idle, k, sentinel, capacity=None, expect=None):
    """what an apply leaves in an out filled with `sentinel` -> (out (rows, k n) int16, report)"""
    outs, report = play_ref(table, packed, used, n, idle, k, capacity, expect)
    full = np.full((len(outs), k * n), sentinel, dtype=np.int16)
    for r, o in enumerate(outs):
        if o is not None:
            full[r] = o
    return full, report


# ---- inputs ---------------------------------------------------------------------------------------------------------

def random_table(n, k, seed, gaps=(0, 3, 1), lead=1, shuffle_offsets=True, dense=False):
    """a random good row of n samples: plays of random lengths at random ascending starts (touching now and then;
    `dense`: every other sample a one-sample play), their codes at offsets with a lead and gaps between them and --
    `shuffle_offsets` -- not in the order of the plays -> (table (count, 3) int32, packed int16, capacity in samples)"""
    rng = np.random.default_rng(seed)
    spans, at = [], 0
    while at < n:
        if dense:
            length, skip = 1, 1
        else:
            length = int(rng.integers(1, max(2, min(n - at, 20) + 1)))
            skip = int(rng.integers(0, 6))                   # 0: the next play touches this one
        length = min(length, n - at)
        spans.append((at, length))
        at += length + skip
        if not dense and rng.integers(0, 4) == 0:
            at += int(rng.integers(0, max(n // 4, 1)))
    if not dense and spans and rng.integers(0, 2):
        spans = spans[1:] if spans[0][0] == 0 and len(spans) > 1 else spans      # rows that start in a gap, too
    order = rng.permutation(len(spans)) if shuffle_offsets else np.arange(len(spans))
    offsets, off, parts = [0] * len(spans), int(lead), []
    if lead:
        parts.append(np.full(k * lead, 0x1111, dtype=np.int16))
    for i, j in enumerate(order):
        offsets[j] = off
        parts.append(rng.integers(-32768, 32768, k * spans[j][1]).astype(np.int16))
        off += spans[j][1]
        g = int(gaps[i % len(gaps)]) if gaps else 0
        if g:
            parts.append(np.full(k * g, 0x2222, dtype=np.int16))
            off += g
    table = np.asarray([[s, l, o] for (s, l), o in zip(spans, offsets)], dtype=np.int32).reshape(-1, 3)
    packed = np.concatenate(parts).astype(np.int16) if parts else np.zeros(0, dtype=np.int16)
    return table, packed, off


def stack_rows(rows, k, max_segments=None, capacity=None):
    """rows: a list of (table, packed, capacity, ...) -> (table (rows, max_segments, 3) int32, packed (rows, k
    capacity) int16, used (rows, 2) int64), padded with entries and codes that no good apply reads"""
    ms = max(len(r[0]) for r in rows) if max_segments is None else max_segments
    cap = max(r[2] for r in rows) if capacity is None else capacity
    table = np.full((len(rows), ms, 3), -7, dtype=np.int32)
    packed = np.full((len(rows), k * cap), 0x3333, dtype=np.int16)
    used = np.zeros((len(rows), 2), dtype=np.int64)
    for i, r in enumerate(rows):
        table[i, :len(r[0])] = r[0]
        packed[i, :len(r[1])] = r[1]
        used[i] = len(r[0]), r[2]
    return table, packed, used
