"""Referee of the segment library (distortion.SegmentLibrary / library_rows, csrc/wfk_segment_library.hip): the
semantics in Python, twice -- a dict keyed on (length, bytes) in order of first occurrence, and a double loop that
compares every segment with every earlier one -- with the rule of the rows that cannot be read and the cut of the
library at lib_capacity, and the builders of the inputs the tests use.

Per row of `count` segments [start, length, offset] over `packed` (k = width codes per sample):
    segments i and j are EQUAL when length_i == length_j and the k length codes at k offset are equal verbatim
    the FIRST of a class is its lowest j; the firsts in ascending j are the slots u = 0, 1, ...
    lib_offset_u = the lengths of the slots before u;  unique = the slots;  lib_kept = the lengths of all slots
    plays[j] = [start_j, length_j, lib_offset of the slot of j];  slots[j] = the slot of j
    library  = the codes of the slots back to back
A row is BAD when count or kept lie outside [0, max_segments] / [0, capacity], or an entry j < count has length <= 0,
offset < 0 or offset + length > capacity: lib_used = [-1, -1], nothing else.  Everything is an integer: every
comparison against this file is exact."""
import numpy as np


def row_is_bad(table, used_row, max_segments, capacity):
    count, kept = int(used_row[0]), int(used_row[1])
    if count < 0 or count > max_segments or kept < 0 or kept > capacity:
        return True
    for j in range(count):
        length, offset = int(table[j, 1]), int(table[j, 2])
        if length <= 0 or offset < 0 or offset + length > capacity:
            return True
    return False


def library_row_dict(table, packed, count, k):
    """one good row by a dict over (length, bytes) -> (plays (count, 3) int32, slots (count,) int32, library int16)"""
    seen, plays, slots, pieces, kept = {}, [], [], [], 0
    for j in range(count):
        start, length, offset = (int(v) for v in table[j])
        codes = packed[k * offset:k * (offset + length)]
        key = (length, codes.tobytes())
        if key not in seen:
            seen[key] = (len(seen), kept)
            pieces.append(codes)
            kept += length
        u, lib_offset = seen[key]
        plays.append([start, length, lib_offset])
        slots.append(u)
    library = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int16)
    return (np.asarray(plays, dtype=np.int32).reshape(-1, 3), np.asarray(slots, dtype=np.int32),
            library.astype(np.int16))


def library_row_loop(table, packed, count, k):
    """the same by the definition: every segment against every earlier one"""
    first = []
    for j in range(count):
        f = j
        for i in range(j):
            if int(table[i, 1]) != int(table[j, 1]):
                continue
            a = packed[k * int(table[i, 2]):k * (int(table[i, 2]) + int(table[i, 1]))]
            b = packed[k * int(table[j, 2]):k * (int(table[j, 2]) + int(table[j, 1]))]
            if np.array_equal(a, b):
                f = i
                break
        first.append(f)
    slot_of, lib_offset, pieces, kept = {}, {}, [], 0
    for j in range(count):
        if first[j] == j:
            slot_of[j], lib_offset[j] = len(slot_of), kept
            pieces.append(packed[k * int(table[j, 2]):k * (int(table[j, 2]) + int(table[j, 1]))])
            kept += int(table[j, 1])
    plays = [[int(table[j, 0]), int(table[j, 1]), lib_offset[first[j]]] for j in range(count)]
    slots = [slot_of[first[j]] for j in range(count)]
    library = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int16)
    return (np.asarray(plays, dtype=np.int32).reshape(-1, 3), np.asarray(slots, dtype=np.int32),
            library.astype(np.int16))


def library_ref(table, packed, used, k=1, capacity=None, form='dict'):
    """table (rows, max_segments, 3) int32, packed (rows, >= k capacity) int16, used (rows, 2) int64 -> (plays, slots,
    library: a list per row (None for a bad row), lib_used int64 (rows, 2))"""
    table, packed, used = np.asarray(table), np.asarray(packed), np.asarray(used)
    rows, max_segments = table.shape[0], table.shape[1]
    capacity = packed.shape[1] // k if capacity is None else capacity
    one = library_row_dict if form == 'dict' else library_row_loop
    plays, slots, library, lib_used = [], [], [], np.zeros((rows, 2), dtype=np.int64)
    for r in range(rows):
        if row_is_bad(table[r], used[r], max_segments, capacity):
            plays.append(None), slots.append(None), library.append(None)
            lib_used[r] = -1
            continue
        p, s, y = one(table[r], packed[r], int(used[r, 0]), k)
        plays.append(p), slots.append(s), library.append(y)
        lib_used[r] = [int(s.max()) + 1 if len(s) else 0, len(y) // k]
    return plays, slots, library, lib_used


def expected_outputs(table, packed, used, k, lib_capacity, sentinels, capacity=None):
    """what an apply leaves in outputs filled with `sentinels` (plays, slots, library) -> (plays (rows, max_segments,
    3), slots (rows, max_segments), library (rows, k lib_capacity), lib_used): the cut is by position"""
    plays, slots, library, lib_used = library_ref(table, packed, used, k, capacity)
    rows, ms = table.shape[0], table.shape[1]
    P = np.full((rows, ms, 3), sentinels[0], dtype=np.int32)
    S = np.full((rows, ms), sentinels[1], dtype=np.int32)
    Y = np.full((rows, k * lib_capacity), sentinels[2], dtype=np.int16)
    for r in range(rows):
        if plays[r] is None:
            continue
        c = len(plays[r])
        P[r, :c], S[r, :c] = plays[r], slots[r]
        q = min(len(library[r]), k * lib_capacity)
        Y[r, :q] = library[r][:q]
    return P, S, Y, lib_used


# ---- inputs ---------------------------------------------------------------------------------------------------------

def shapes_of(lengths, k, seed):
    """one random shape of k length codes per length"""
    rng = np.random.default_rng(seed)
    return [rng.integers(-32768, 32768, k * int(n)).astype(np.int16) for n in lengths]


def variant(shape, at, flip=1):
    """the shape with the bits `flip` of its code `at` (negative: from the end) turned over"""
    v = shape.copy()
    v.view(np.uint16)[at] ^= np.uint16(flip)
    return v


def row_of(pieces, k, gaps=None, lead=0, align=1):
    """a row that plays `pieces` (arrays of k length codes) in order: -> (table (count, 3) int32, packed int16, kept).
    `gaps`: samples of filler between consecutive pieces in packed (so offsets need not be the running sum: the
    library reads offsets, it does not assume them), `lead`: samples of filler before the first, `align`: every
    offset is `lead` past a multiple of it."""
    table, parts, off, start = [], [], int(lead), 0
    if lead:
        parts.append(np.full(k * lead, 0x1111, dtype=np.int16))
    for i, p in enumerate(pieces):
        n = len(p) // k
        pad = -(off - lead) % align
        if pad:
            parts.append(np.full(k * pad, 0x4444, dtype=np.int16))
            off += pad
        table.append([start, n, off])
        parts.append(p)
        off += n
        start += n + 3
        g = 0 if gaps is None else int(gaps[i % len(gaps)])
        if g:
            parts.append(np.full(k * g, 0x2222, dtype=np.int16))
            off += g
    packed = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)
    return np.asarray(table, dtype=np.int32).reshape(-1, 3), packed.astype(np.int16), off


def drawn_row(count, shapes, k, seed, gaps=None, lead=0):
    """a row of `count` segments drawn at random from `shapes` -> (table, packed, kept, the draw)"""
    rng = np.random.default_rng(seed)
    draw = rng.integers(0, len(shapes), count) if count else np.zeros(0, dtype=np.int64)
    return row_of([shapes[d] for d in draw], k, gaps, lead) + (draw,)


def stack_rows(rows, k, max_segments=None, capacity=None):
    """rows: a list of (table, packed, kept, ...) -> (table (rows, max_segments, 3) int32, packed (rows, k capacity)
    int16, used (rows, 2) int64), padded with entries and codes that no good apply reads"""
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
