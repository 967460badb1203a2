"""The segment library on the device (distortion.SegmentLibrary / library_rows, csrc/wfk_segment_library.hip) against
the referee tests/segment_library_ref.py, the Python statement of the semantics.  Plays, slots, library codes and
totals are integers: every comparison here is exact.  Every apply goes through `check`, which gives the stage windows
of wider sentinel-filled tensors at given leads and compares the WHOLE of them with what the referee says -- the entries
and codes the stage owes, and the sentinel everywhere else -- fills lib_used with garbage first, compares the inputs as
bits afterwards, applies a second time and runs the sizing pass; and does all of that with the full hash and with
WFK_SEGLIB_HASH_BITS in {0, 1, 4}, which must give the same bits.  The cases that do not go through `check` (streams,
graph replay, far rows, download, the refusals, the end-to-end chain, the C consumer) make one plan per setting too.
Inputs are built directly as table / packed / used, so the shapes are the smallest that can go wrong."""
import contextlib
import os
import subprocess

import numpy as np
import pytest
import torch

import graph_replay
import segment_library_ref as ref
from row_windows import FarWindow, bits_equal, free_far_arena
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP, SS, SL = 0x5EC7AB1E, 0x51075, -23101       # what plays, slots and the library rows hold before an apply
SENTINELS = (SP, SS, SL)
GARBAGE = 0x5a5a5a5a5a
ALL_BITS = (None, 0, 1, 4)
LENGTHS = [1, 7, 8, 9, 63, 64, 65, 511, 513, 4097, 20001]


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}; last at {tuple(bad[-1])}')


@contextlib.contextmanager
def hash_bits(bits):
    """WFK_SEGLIB_HASH_BITS, read when a plan is made"""
    old = os.environ.get('WFK_SEGLIB_HASH_BITS')
    try:
        if bits is None:
            os.environ.pop('WFK_SEGLIB_HASH_BITS', None)
        else:
            os.environ['WFK_SEGLIB_HASH_BITS'] = str(bits)
        yield
    finally:
        if old is None:
            os.environ.pop('WFK_SEGLIB_HASH_BITS', None)
        else:
            os.environ['WFK_SEGLIB_HASH_BITS'] = old


def library_of(rows, ms, cap, k, lib_capacity=None, bits=None):
    """a SegmentLibrary whose device plan is made -- and the switch read -- while WFK_SEGLIB_HASH_BITS is `bits`"""
    lib = distortion.SegmentLibrary(rows, ms, cap, k, lib_capacity)
    with hash_bits(bits):
        names = [lib.kernel_name(i) for i in range(5)]
    tail = '' if bits is None or bits >= 64 else f' [hash bits {bits}]'
    assert names == ['seglib_hash' + tail, 'seglib_match' + tail, 'seglib_scan', 'seglib_copy', ''], names
    return lib


def table_window(rows, ms, lead, fill):
    """-> (the wide (rows, 3 ms + 8) int32 tensor, its window (rows, ms, 3) `lead` ints in)"""
    wide = torch.full((rows, 3 * ms + 8), fill, dtype=torch.int32, device=dev())
    return wide, wide.as_strided((rows, ms, 3), (wide.stride(0), 3, 1), lead)


def widen(a, lead, extra, fill):
    """host (rows, n) -> host (rows, n + extra) filled with `fill`, `a` at column `lead`"""
    w = np.full((a.shape[0], a.shape[1] + extra), fill, dtype=a.dtype)
    w[:, lead:lead + a.shape[1]] = a
    return w


def check(table, packed, used, k=1, lib_capacity=None, what='', table_lead=1, packed_lead=5, plays_lead=2,
          slots_lead=3, library_lead=3, capacity=None):
    """one library per setting of the hash bits, windows at the given leads (elements) into wider tensors, two applies
    and the sizing pass against the referee; the inputs compared as bits afterwards -> (plays, slots, library,
    lib_used) of the referee"""
    rows, ms = table.shape[0], table.shape[1]
    cap = packed.shape[1] // k if capacity is None else capacity
    libcap = cap if lib_capacity is None else lib_capacity
    wide_t, tw = table_window(rows, ms, table_lead, -1)
    tw.copy_(torch.from_numpy(table))
    wide_y = torch.full((rows, k * cap + 24), -1, dtype=torch.int16, device=dev())
    yw = wide_y[:, packed_lead:packed_lead + k * cap]
    yw.copy_(torch.from_numpy(packed[:, :k * cap]))
    ud = torch.from_numpy(used).to(dev())
    before = [x.cpu().numpy().copy() for x in (wide_t, wide_y, ud)]
    want_p, want_s, want_l, want_used = ref.expected_outputs(table, packed, used, k, libcap, SENTINELS, cap)
    full_p = widen(want_p.reshape(rows, 3 * ms), plays_lead, 8, SP)
    full_s = widen(want_s, slots_lead, 8, SS)
    full_l = widen(want_l, library_lead, 24, SL)
    for bits in ALL_BITS:
        lib = library_of(rows, ms, cap, k, lib_capacity, bits)
        tag = f'{what} [bits {bits}]'
        try:
            wide_p, pw = table_window(rows, ms, plays_lead, SP)
            wide_s = torch.full((rows, ms + 8), SS, dtype=torch.int32, device=dev())
            wide_l = torch.full((rows, k * libcap + 24), SL, dtype=torch.int16, device=dev())
            sw, lw = wide_s[:, slots_lead:slots_lead + ms], wide_l[:, library_lead:library_lead + k * libcap]
            lib_used = torch.full((rows, 2), GARBAGE, dtype=torch.int64, device=dev())
            for turn in ('first apply', 'second apply'):
                p, s, y, u = lib.apply_torch(tw, yw, ud, plays=pw, slots=sw, library=lw, lib_used=lib_used)
                assert (p.data_ptr(), s.data_ptr(), y.data_ptr(), u.data_ptr()) == \
                    (pw.data_ptr(), sw.data_ptr(), lw.data_ptr(), lib_used.data_ptr())
                assert tuple(p.shape) == (rows, ms, 3) and tuple(s.shape) == (rows, ms) and tuple(y.shape) == (rows, k * libcap)
                same(lib_used.cpu().numpy(), want_used, f'{tag}: lib_used, {turn}')
                same(wide_p.cpu().numpy(), full_p, f'{tag}: plays, {turn}')
                same(wide_s.cpu().numpy(), full_s, f'{tag}: slots, {turn}')
                same(wide_l.cpu().numpy(), full_l, f'{tag}: library, {turn}')
                lib_used.fill_(-GARBAGE)
            same(lib.measure_torch(tw, yw, ud, lib_used=lib_used).cpu().numpy(), want_used, f'{tag}: sizing pass')
            same(lib.measure_torch(tw, yw, ud).cpu().numpy(), want_used, f'{tag}: sizing pass, allocated')
            for x, b, name in zip((wide_t, wide_y, ud), before, ('table', 'packed', 'used')):
                assert bits_equal(x.cpu().numpy(), b), f'{tag}: {name} was written'
            same(wide_p.cpu().numpy(), full_p, f'{tag}: plays after the sizing pass')
            same(wide_l.cpu().numpy(), full_l, f'{tag}: library after the sizing pass')
        finally:
            lib.close()
    return ref.library_ref(table, packed, used, k, cap)


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('length', LENGTHS)
def test_lengths_at_odd_and_aligned_offsets(length, k):
    s, other = ref.shapes_of([length, length], k, 3 * length + k)
    pieces = [s, ref.variant(s, -1), other, s, other, ref.variant(s, 0, 0x100)]
    rows = [ref.row_of(pieces, k, lead=1), ref.row_of(pieces, k, align=8), ref.row_of(pieces, k, lead=3, align=8),
            ref.row_of(pieces, k, gaps=[0, 1, 2, 5])]
    assert np.all(rows[1][0][:, 2] % 8 == 0) and np.all(rows[2][0][:, 2] % 8 == 3) and rows[0][0][0, 2] == 1
    table, packed, used = ref.stack_rows(rows, k)
    _, slots, _, lib_used = check(table, packed, used, k, what=f'length {length} k={k}')
    assert lib_used.tolist() == [[4, 4 * length]] * 4 and all(s.tolist() == [0, 1, 2, 0, 2, 3] for s in slots)


@pytest.mark.parametrize('k', [1, 2])
def test_segments_that_differ_in_one_place(k):
    for length in (1, 9, 64, 513):
        s = ref.shapes_of([length], k, 40 + length)[0]
        pieces = [s, ref.variant(s, 0, 0x4000), ref.variant(s, -1, 2), ref.variant(s, (k * length) // 2, 0x10),
                  ref.variant(s, 0, 1), ref.variant(s, -1, 0x8000), s]      # first, last, middle, marker bits 0 and 15
        if k == 2:
            pieces += [ref.variant(s, -2, 4), ref.variant(s, -1, 4)]        # either code of the last sample
        distinct = len({p.tobytes() for p in pieces})
        for lead in (0, 1):
            table, packed, used = ref.stack_rows([ref.row_of(pieces, k, lead=lead), ref.row_of(pieces[::-1], k, lead=lead)], k)
            _, slots, _, lib_used = check(table, packed, used, k, what=f'one place, length {length} k={k} lead {lead}')
            assert lib_used[:, 0].tolist() == [distinct] * 2 and slots[0][6] == 0 and distinct == len(pieces) - 1


@pytest.mark.parametrize('k', [1, 2])
def test_a_prefix_is_another_segment(k):
    s = ref.shapes_of([70], k, 50)[0]
    pieces = [s, s[:k * 64], s[:k * 8], s, s[:k * 64], s[:k * 1], s[:k * 8], s[:k * 69]]
    table, packed, used = ref.stack_rows([ref.row_of(pieces, k, lead=1), ref.row_of(pieces[::-1], k, align=8)], k)
    _, slots, _, lib_used = check(table, packed, used, k, what=f'prefix k={k}')
    assert slots[0].tolist() == [0, 1, 2, 0, 1, 3, 2, 4] and lib_used[0].tolist() == [5, 70 + 64 + 8 + 1 + 69]


@pytest.mark.parametrize('k', [1, 2])
def test_one_shape_at_every_pair_of_alignments(k):
    s, other = ref.shapes_of([37, 37], k, 60)
    cap = 200
    table = np.zeros((64, 3, 3), dtype=np.int32)
    packed = np.full((64, k * cap), 0x3333, dtype=np.int16)
    used = np.zeros((64, 2), dtype=np.int64)
    for a in range(8):
        for b in range(8):
            r = 8 * a + b
            offsets = (a, 48 + b, 96 + (a + b) % 8)
            for j, (o, piece) in enumerate(zip(offsets, (s, s, other))):
                table[r, j] = [50 * j, 37, o]
                packed[r, k * o:k * (o + 37)] = piece
            used[r] = 3, 140
    for packed_lead in (0, 1):
        _, slots, _, lib_used = check(table, packed, used, k, what=f'alignments k={k}', packed_lead=packed_lead)
        assert lib_used.tolist() == [[2, 74]] * 64 and all(s.tolist() == [0, 0, 1] for s in slots)


@pytest.mark.parametrize('c', [0, 1, 63, 64, 65, 129, 4097])
def test_counts(c):
    k = 1 + c % 2
    for extra in (0, 3):
        one = ref.shapes_of([5], k, c)
        different = ref.shapes_of([3 + d % 7 for d in range(max(c, 1))], k, c + 1)
        sixteen = ref.shapes_of([2 + d for d in range(16)], k, c + 2)
        rows = [ref.drawn_row(c, one, k, 1, lead=1), ref.drawn_row(c, different, k, 2), ref.drawn_row(c, sixteen, k, 3, lead=1),
                ref.row_of(different[:c], k)]
        table, packed, used = ref.stack_rows(rows, k, max_segments=c + extra)
        _, _, _, lib_used = check(table, packed, used, k, what=f'c={c} max_segments={c + extra}')
        assert lib_used[0, 0] == min(c, 1) and lib_used[3, 0] == c and lib_used[2, 0] == (16 if c >= 129 else lib_used[2, 0])
        assert lib_used[3, 1] == used[3, 1] and lib_used[2, 0] <= 16     # all different: the library is the packed side


@pytest.mark.parametrize('k', [1, 2])
def test_cuts_are_by_position_and_report_the_true_totals(k):
    shapes = ref.shapes_of([20, 33, 8, 41], k, 70)
    rows = [ref.drawn_row(40, shapes, k, 71, lead=1), ref.drawn_row(40, shapes[:2], k, 72), ref.drawn_row(3, shapes[3:], k, 73)]
    table, packed, used = ref.stack_rows(rows, k)
    _, _, _, lib_used = ref.library_ref(table, packed, used, k)
    kept = int(lib_used[:, 1].max())
    assert lib_used.tolist() == [[4, 102], [2, 53], [1, 41]]
    for libcap in (0, kept - 1, kept, 30, 53, 5):                          # 30: in mid-slot of rows 0 and 1
        got = check(table, packed, used, k, lib_capacity=libcap, what=f'lib_capacity={libcap} k={k}',
                    library_lead=libcap % 8)
        assert np.array_equal(got[3], lib_used)


def test_each_output_alone():
    k, shapes = 2, ref.shapes_of([9, 17, 30], 2, 80)
    rows = [ref.drawn_row(20, shapes, k, 81, lead=1), ref.drawn_row(11, shapes, k, 82)]
    table, packed, used = ref.stack_rows(rows, k, max_segments=22)
    ms, cap = 22, packed.shape[1] // k
    want_p, want_s, want_l, want_used = ref.expected_outputs(table, packed, used, k, cap, SENTINELS)
    td, yd, ud = (torch.from_numpy(x).to(dev()) for x in (table, packed, used))
    for bits in ALL_BITS:
        lib = library_of(2, ms, cap, k, None, bits)
        plan = lib._plan()
        for which in range(4):                                              # plays, slots, library, none: the sizing pass
            p = torch.full((2, ms, 3), SP, dtype=torch.int32, device=dev())
            s = torch.full((2, ms), SS, dtype=torch.int32, device=dev())
            y = torch.full((2, k * cap), SL, dtype=torch.int16, device=dev())
            u = torch.full((2, 2), GARBAGE, dtype=torch.int64, device=dev())
            plan.apply(td.data_ptr(), 3 * ms, yd.data_ptr(), k * cap, ud.data_ptr(),
                       p.data_ptr() if which == 0 else None, 3 * ms, s.data_ptr() if which == 1 else None, ms,
                       y.data_ptr() if which == 2 else None, k * cap, u.data_ptr())
            torch.cuda.synchronize()
            same(u.cpu().numpy(), want_used, f'output {which} alone: lib_used')
            same(p.cpu().numpy(), want_p if which == 0 else np.full_like(want_p, SP), f'output {which} alone: plays')
            same(s.cpu().numpy(), want_s if which == 1 else np.full_like(want_s, SS), f'output {which} alone: slots')
            same(y.cpu().numpy(), want_l if which == 2 else np.full_like(want_l, SL), f'output {which} alone: library')
        lib.close()


def test_every_lead_of_the_sides():
    k, shapes = 1, ref.shapes_of([9, 16, 25, 40], 1, 90)
    rows = [ref.drawn_row(30, shapes, k, 91, lead=1), ref.drawn_row(30, shapes, k, 92, gaps=[0, 1, 3])]
    table, packed, used = ref.stack_rows(rows, k)
    for lead in range(8):
        check(table, packed, used, k, what=f'packed lead {lead}', packed_lead=lead, library_lead=(3 * lead + 1) % 8,
              table_lead=lead % 4, plays_lead=(lead + 1) % 4, slots_lead=(lead + 2) % 4)
    for library_lead in range(8):
        for k2 in (1, 2):
            t2, p2, u2 = ref.stack_rows([ref.drawn_row(12, ref.shapes_of([9, 16, 25], k2, 93), k2, 94, lead=1)] * 2, k2)
            check(t2, p2, u2, k2, what=f'library lead {library_lead} k={k2}', library_lead=library_lead, packed_lead=0)


def bad_rows_case(k=1):
    """-> (table, packed, used, capacity): good rows 0, 2, 4, ... with a row that cannot be read after each"""
    shapes = ref.shapes_of([4, 4, 6], k, 100)
    good = [ref.drawn_row(5, shapes, k, 101 + i, lead=i % 2) for i in range(11)]
    rows = []
    for g in good[:10]:
        rows += [g, good[10]]
    cap = 40
    table, packed, used = ref.stack_rows(rows, k, max_segments=6, capacity=cap)
    used[1, 0] = 7                                                          # count = max_segments + 1
    used[3, 1] = cap + 1
    used[5] = -1, 3
    used[7] = 2, -1
    table[9, 2, 1] = 0
    table[11, 4, 1] = -1
    table[13, 0, 2] = -1
    table[15, 3] = [7, 6, cap - 5]                                          # offset + length = capacity + 1
    table[17, 1, 1:] = 2**31 - 1
    used[19, 0] = 2**40
    return table, packed, used, cap


@pytest.mark.parametrize('k', [1, 2])
def test_rows_that_cannot_be_read_are_reported_and_left_alone(k):
    table, packed, used, cap = bad_rows_case(k)
    _, _, library, lib_used = check(table, packed, used, k, what=f'bad rows k={k}', capacity=cap)
    assert np.all(lib_used[1::2] == -1) and np.all(lib_used[0::2, 0] >= 1) and all(y is None for y in library[1::2])
    table[15, 3] = [7, 6, cap - 6]                                          # ... = capacity: the row is good
    assert check(table, packed, used, k, what=f'to the end of the row k={k}', capacity=cap)[3][15, 0] > 0


def test_five_applies_agree_to_the_bit():
    k = 2
    one = ref.shapes_of([24], k, 110)
    rows = [ref.drawn_row(4097, one, k, 1, lead=1), ref.drawn_row(4097, ref.shapes_of([3, 5, 8], k, 111), k, 2)]
    table, packed, used = ref.stack_rows(rows, k)
    want = ref.expected_outputs(table, packed, used, k, packed.shape[1] // k, SENTINELS)
    td, yd, ud = (torch.from_numpy(x).to(dev()) for x in (table, packed, used))
    for bits in ALL_BITS:
        lib = library_of(2, 4097, packed.shape[1] // k, k, None, bits)
        for turn in range(5):
            got = lib.apply_torch(td, yd, ud, plays=torch.full((2, 4097, 3), SP, dtype=torch.int32, device=dev()),
                                  slots=torch.full((2, 4097), SS, dtype=torch.int32, device=dev()),
                                  library=torch.full((2, packed.shape[1]), SL, dtype=torch.int16, device=dev()))
            for g, w, name in zip(got, want, ('plays', 'slots', 'library', 'lib_used')):
                same(g.cpu().numpy(), w, f'apply {turn} bits {bits}: {name}')
        lib.close()
    assert want[3].tolist() == [[1, 24], [3, 16]]


@pytest.mark.parametrize('bits', ALL_BITS)
def test_side_stream_equals_default_stream(bits):
    k, shapes = 2, ref.shapes_of([30, 64, 100], 2, 120)
    rows = [ref.drawn_row(200, shapes, k, 121 + i, lead=i) for i in range(3)]
    table, packed, used = ref.stack_rows(rows, k)
    cap = packed.shape[1] // k
    want = ref.expected_outputs(table, packed, used, k, cap, SENTINELS)
    lib = library_of(3, 200, cap, k, None, bits)
    outs = []
    side = torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), side):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            td, yd, ud = (torch.from_numpy(x).to(dev()) for x in (table, packed, used))
            got = lib.apply_torch(td, yd, ud, plays=torch.full((3, 200, 3), SP, dtype=torch.int32, device=dev()),
                                  slots=torch.full((3, 200), SS, dtype=torch.int32, device=dev()),
                                  library=torch.full((3, k * cap), SL, dtype=torch.int16, device=dev()))
            outs.append(tuple(x + 0 for x in got))                          # produced and consumed on that stream
        stream.synchronize()
    for name, got in zip(('default', 'side'), outs):
        for g, w, what in zip(got, want, ('plays', 'slots', 'library', 'lib_used')):
            same(g.cpu().numpy(), w, f'{name} stream, {what}')
    lib.close()


@pytest.mark.parametrize('bits', ALL_BITS)
def test_graph_replay_on_other_inputs(bits):
    k, ms, cap = 2, 40, 900
    feeds, wants = [], []
    for seed, D in ((130, 3), (131, 1), (132, 6)):
        shapes = ref.shapes_of([5 + 7 * d for d in range(D)], k, seed)
        rows = [ref.drawn_row(30 + i, shapes, k, seed + i, lead=i) for i in range(3)]
        table, packed, used = ref.stack_rows(rows, k, max_segments=ms, capacity=cap)
        if seed == 131:
            table[1, 4, 2] = cap                                            # a row that turns bad, and good again
        feeds.append([table, packed, used])
        wants.append(ref.expected_outputs(table, packed, used, k, cap, (0, 0, 0)))
    lib = library_of(3, ms, cap, k, None, bits)
    td = torch.empty((3, ms, 3), dtype=torch.int32, device=dev())
    yd = torch.empty((3, k * cap), dtype=torch.int16, device=dev())
    ud = torch.empty((3, 2), dtype=torch.int64, device=dev())
    plays = torch.empty((3, ms, 3), dtype=torch.int32, device=dev())
    slots = torch.empty((3, ms), dtype=torch.int32, device=dev())
    library = torch.empty((3, k * cap), dtype=torch.int16, device=dev())
    lib_used = torch.empty((3, 2), dtype=torch.int64, device=dev())

    def run():
        lib.apply_torch(td, yd, ud, plays=plays, slots=slots, library=library, lib_used=lib_used)

    got = graph_replay.replay(run, [td, yd, ud], feeds, [plays, slots, library, lib_used])
    for turn, ((p, s, y, u), feed) in enumerate(zip(got, feeds)):
        want_p, want_s, want_l, want_used = ref.expected_outputs(*feed, k, cap, SENTINELS)
        same(u, want_used, f'replay {turn}: lib_used')
        # what the stage owes, element for element; everything else still holds what the helper filled it with
        for g, w, fill, name in ((p, want_p, SP, 'plays'), (s, want_s, SS, 'slots'), (y, want_l, SL, 'library')):
            owed = w != fill
            same(g[owed], w[owed], f'replay {turn}: {name}')
            assert graph_replay.sentinels_left(g) == int((~owed).sum()) + graph_replay.sentinels_left(w[owed]), \
                f'replay {turn}: {name} written outside what the stage owes'
    assert [w[3][1].tolist() == [-1, -1] for w in wants] == [False, True, False]
    assert len({tuple(w[3].reshape(-1)) for w in wants}) == 3
    lib.close()


def test_far_rows():
    """packed rows more than 2^32 codes apart: plays, slots, the library and the totals as the referee has them, every
    guard of the arena untouched, the packed codes bit for bit what was put there"""
    k, cap = 1, 2**17 - 3
    shapes = ref.shapes_of([300, 777, 1024], k, 140)
    rows = [ref.drawn_row(130, shapes, k, 141 + i, lead=1 + i) for i in range(2)]
    table, packed, used = ref.stack_rows(rows, k, capacity=cap)
    want = ref.expected_outputs(table, packed, used, k, cap, SENTINELS)
    assert want[3].tolist() == [[3, 2101]] * 2
    try:
        src = FarWindow(cap, np.int16, packed)
        td, ud = torch.from_numpy(table).to(dev()), torch.from_numpy(used).to(dev())
        for bits in ALL_BITS:
            lib = library_of(2, 130, cap, k, None, bits)
            try:
                got = lib.apply_torch(td, src.win, ud, plays=torch.full((2, 130, 3), SP, dtype=torch.int32, device=dev()),
                                      slots=torch.full((2, 130), SS, dtype=torch.int32, device=dev()),
                                      library=torch.full((2, cap), SL, dtype=torch.int16, device=dev()))
                for g, w, name in zip(got, want, ('plays', 'slots', 'library', 'lib_used')):
                    same(g.cpu().numpy(), w, f'far packed rows, bits {bits}: {name}')
            finally:
                lib.close()
        src.assert_holds(packed)
        del src
    finally:
        free_far_arena()


@pytest.mark.parametrize('bits', ALL_BITS)
def test_download_and_library_rows(bits):
    k, shapes = 2, ref.shapes_of([16, 48, 80], 2, 150)
    rows = [ref.drawn_row(25, shapes, k, 151, lead=1), ref.drawn_row(0, shapes, k, 152), ref.drawn_row(9, shapes[:1], k, 153)]
    table, packed, used = ref.stack_rows(rows, k)
    cap = packed.shape[1] // k
    plays, slots, library, lib_used = ref.library_ref(table, packed, used, k)
    td, yd, ud = (torch.from_numpy(x).to(dev()) for x in (table, packed, used))
    lib = library_of(3, 25, cap, k, None, bits)
    out = lib.apply_torch(td, yd, ud)
    got = lib.download(*out, ud)
    assert len(got) == 3 and lib_used[1].tolist() == [0, 0]
    for r, (p, s, y) in enumerate(got):
        same(p, plays[r], f'download: plays of row {r}')
        same(s, slots[r], f'download: slots of row {r}')
        same(y, library[r], f'download: library of row {r}')
    lib.close()
    kept = int(lib_used[:, 1].max())
    tight = library_of(3, 25, cap, k, kept - 1, bits)
    with pytest.raises(ValueError, match=f'row {int(lib_used[:, 1].argmax())} overflowed'):
        tight.download(*tight.apply_torch(td, yd, ud), ud)
    tight.close()
    exact = library_of(3, 25, cap, k, kept, bits)
    for (p, s, y), wp, wy in zip(exact.download(*exact.apply_torch(td, yd, ud), ud), plays, library):
        same(p, wp, 'download at the exact size: plays')
        same(y, wy, 'download at the exact size: library')
    ud2 = ud.clone()
    ud2[2, 0] = 26
    with pytest.raises(ValueError, match='row 2 could not be read'):
        exact.download(*exact.apply_torch(td, yd, ud2), ud2)
    exact.close()
    segments = [(r[0], r[1]) for r in rows]
    with hash_bits(bits):                                                            # (library_rows makes its own plan)
        got_rows = distortion.library_rows(segments, width=k)
    for r, (p, s, y) in enumerate(got_rows):                                         # NumPy in, NumPy out
        same(p, plays[r], f'library_rows: plays of row {r}')
        same(s, slots[r], f'library_rows: slots of row {r}')
        same(y, library[r], f'library_rows: library of row {r}')
    broken = (rows[0][0].copy(), rows[0][1])
    broken[0][3, 2] = len(rows[0][1])
    with hash_bits(bits), pytest.raises(ValueError, match='library_rows: row 1: the table does not fit'):
        distortion.library_rows([segments[0], broken], width=k)


@pytest.mark.parametrize('bits', ALL_BITS)
def test_refused_tensors(bits):
    rows, k, ms, cap = 2, 2, 6, 64
    lib = library_of(rows, ms, cap, k, 32, bits)
    table = torch.zeros((rows, ms, 3), dtype=torch.int32, device=dev())
    packed = torch.zeros((rows, k * cap), dtype=torch.int16, device=dev())
    used = torch.zeros((rows, 2), dtype=torch.int64, device=dev())
    plays = torch.zeros((rows, ms, 3), dtype=torch.int32, device=dev())
    slots = torch.zeros((rows, ms), dtype=torch.int32, device=dev())
    library = torch.zeros((rows, k * 32), dtype=torch.int16, device=dev())
    lib_used = torch.full((rows, 2), 5, dtype=torch.int64, device=dev())
    lib.apply_torch(table, packed, used, plays=plays, slots=slots, library=library, lib_used=lib_used)   # fine
    torch.cuda.synchronize()
    assert not lib_used.cpu().numpy().any()
    lib_used.fill_(5)
    A = lib.apply_torch
    for bad in (table[:1], table[:, :ms - 1], table.to(torch.int64), table.cpu(), table.view(rows, 3 * ms),
                table.permute(0, 2, 1).contiguous().permute(0, 2, 1)):
        with pytest.raises(ValueError, match='expected table'):
            A(bad, packed, used)
        with pytest.raises(ValueError, match='expected table'):
            lib.measure_torch(bad, packed, used)
        with pytest.raises(ValueError, match='expected plays'):
            A(table, packed, used, plays=bad)
    for bad in (packed[:1], packed[:, :k * cap - 1], packed.to(torch.int32), packed.cpu(), packed.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected packed'):
            A(table, bad, used)
    for bad in (library[:1], library[:, :k * 32 - 1], library.to(torch.int32), library.cpu()):
        with pytest.raises(ValueError, match='expected library'):
            A(table, packed, used, library=bad)
    for bad in (slots[:1], slots[:, :ms - 1], slots.to(torch.int64), slots.cpu(), slots.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected slots'):
            A(table, packed, used, slots=bad)
    for bad in (used[:1], used.view(-1), used.to(torch.int32), used.cpu(), None,
                torch.zeros((rows, 3), dtype=torch.int64, device=dev())[:, :2]):
        with pytest.raises(ValueError, match='expected used'):
            A(table, packed, bad)
        if bad is not None:
            with pytest.raises(ValueError, match='expected lib_used'):
                A(table, packed, used, lib_used=bad)
            with pytest.raises(ValueError, match='expected lib_used'):
                lib.measure_torch(table, packed, used, lib_used=bad)
    as_table = packed.view(-1)[:rows * ms * 6].view(torch.int32).view(rows, ms, 3)
    as_slots = packed.view(-1)[:rows * ms * 2].view(torch.int32).view(rows, ms)
    as_report = packed.view(-1)[8:8 + 8 * rows].view(torch.int64).view(rows, 2)
    for kw, message in ((dict(library=packed), 'library overlaps packed'), (dict(plays=table), 'plays overlaps table'),
                        (dict(plays=as_table), 'plays overlaps packed'), (dict(slots=as_slots), 'slots overlaps packed'),
                        (dict(slots=table.view(rows, 3 * ms)[:, :ms]), 'slots overlaps table'),
                        (dict(slots=plays.view(rows, 3 * ms)[:, :ms], plays=plays), 'slots overlaps plays'),
                        (dict(plays=library.view(-1)[:rows * ms * 6].view(torch.int32).view(rows, ms, 3), library=library),
                         'plays overlaps library'),
                        (dict(slots=used.view(torch.int32)[:1].expand(rows, -1)[:, :ms]), 'expected slots'),
                        (dict(lib_used=used), 'lib_used overlaps'), (dict(lib_used=as_report), 'lib_used overlaps'),
                        (dict(lib_used=plays.view(-1)[:4 * rows].view(torch.int64).view(rows, 2), plays=plays),
                         'lib_used overlaps')):
        with pytest.raises(ValueError, match=message):
            A(table, packed, used, **kw)
    with pytest.raises(ValueError, match='lib_used overlaps'):
        lib.measure_torch(table, packed, used, lib_used=as_report)
    torch.cuda.synchronize()
    assert np.all(lib_used.cpu().numpy() == 5) and not plays.cpu().numpy().any() and not library.cpu().numpy().any()
    lib.close()
    empty = library_of(rows, 0, 0, k, None, bits)                                # nothing to hold: lib_used zeroed
    p, s, y, u = empty.apply_torch(table[:, :0], packed[:, :0], used)
    assert tuple(p.shape) == (rows, 0, 3) and tuple(s.shape) == (rows, 0) and tuple(y.shape) == (rows, 0)
    assert not u.cpu().numpy().any() and empty.download(p, s, y, u, used)[1][0].shape == (0, 3)
    used2 = used.clone()
    used2[1, 0] = 1                                                              # a segment where there is room for none
    assert empty.measure_torch(table[:, :0], packed[:, :0], used2).cpu().numpy().tolist() == [[0, 0], [-1, -1]]
    empty.close()


@pytest.mark.parametrize('bits', ALL_BITS)
def test_library_refuses_a_bad_apply(bits):
    """the C side's own checks of an apply, through the raw pointers; nothing is launched"""
    rows, k, ms, cap = 2, 1, 6, 64
    lib = library_of(rows, ms, cap, k, None, bits)
    table = torch.zeros((rows, ms, 3), dtype=torch.int32, device=dev())
    packed = torch.zeros((rows, cap), dtype=torch.int16, device=dev())
    used = torch.zeros((rows, 2), dtype=torch.int64, device=dev())
    plays = torch.zeros((rows, ms, 3), dtype=torch.int32, device=dev())
    slots = torch.zeros((rows, ms), dtype=torch.int32, device=dev())
    library = torch.zeros((rows, cap), dtype=torch.int16, device=dev())
    lib_used = torch.full((rows, 2), 5, dtype=torch.int64, device=dev())
    t, y, u, p, s, l, r = (x.data_ptr() for x in (table, packed, used, plays, slots, library, lib_used))
    plan = lib._plan()
    plan.apply(t, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l, cap, r)                # fine
    torch.cuda.synchronize()
    assert not lib_used.cpu().numpy().any()
    lib_used.fill_(5)
    for args, message in (((t, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l, cap, None), 'lib_used is null'),
                          ((t, 3 * ms, y, cap, None, p, 3 * ms, s, ms, l, cap, r), 'used is null'),
                          ((None, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l, cap, r), 'null'),
                          ((t, 3 * ms, None, cap, u, None, 0, None, 0, None, 0, r), 'null'),
                          ((t, 3 * ms - 1, y, cap, u, p, 3 * ms, s, ms, l, cap, r), 'table row stride smaller'),
                          ((t, 3 * ms, y, cap - 1, u, p, 3 * ms, s, ms, l, cap, r), 'packed row stride smaller'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms - 1, s, ms, l, cap, r), 'plays row stride smaller'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, s, ms - 1, l, cap, r), 'slots row stride smaller'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l, cap - 1, r), 'library row stride smaller'),
                          ((t + 2, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l, cap, r), 'not aligned'),
                          ((t, 3 * ms, y + 1, cap, u, p, 3 * ms, s, ms, l, cap, r), 'not aligned'),
                          ((t, 3 * ms, y, cap, u + 4, p, 3 * ms, s, ms, l, cap, r), 'not aligned'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l + 1, cap, r), 'not aligned'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l, cap, r + 4), 'counts are not aligned'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, s, ms, y + 2, cap, r), 'library overlaps packed'),
                          ((t, 3 * ms, y, cap, u, t + 4, 3 * ms, s, ms, l, cap, r), 'plays overlaps table'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, u, ms, l, cap, r), 'slots overlaps used'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, p + 4, ms, l, cap, r), 'slots overlaps plays'),
                          ((t, 3 * ms, y, cap, u, l + 4, 3 * ms, s, ms, l, cap, r), 'plays overlaps library'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l, cap, u), 'counts overlaps used'),
                          ((t, 3 * ms, y, cap, u, p, 3 * ms, s, ms, l, cap, p + 8), 'counts overlaps plays'),
                          ((t, 3 * ms, y, cap, u, None, 0, None, 0, None, 0, y + 8), 'counts overlaps packed'),
                          ((t, 3 * ms - 1, y, cap, u, None, 0, None, 0, None, 0, r), 'table row stride smaller')):
        with pytest.raises(_engine.EngineError, match=message):
            plan.apply(*args)
    torch.cuda.synchronize()
    assert np.all(lib_used.cpu().numpy() == 5) and not plays.cpu().numpy().any() and not library.cpu().numpy().any()
    lib.close()


def test_end_to_end_gates_to_a_library():
    """the README chain: I/Q pairs of pulses sampled at 2 GS/s -> 14-bit codes with the switch marker in bit 0 -> cut in
    granules of 16 samples -> the library: expand_segments(plays_r, library_r, ...) gives pair_codes again, and the
    referee gives the same library.  No particular `unique`: whether two sampled pulses round to the same codes is the
    sampler's business."""
    from waveforms_amd import cosPulse, gaussian
    from waveforms_amd._sampling import BatchSampler
    n, rate, pairs, lead, trail = 8000, 2e9, 3, 20, 10
    starts = [200e-9, 900e-9, 1700e-9, 2600e-9]
    chans = []
    for p in range(pairs):
        i_row = sum(((gaussian(40e-9 + 10e-9 * p) >> t0) for t0 in starts[1:]), gaussian(40e-9) >> starts[0]) * 0.8
        q_row = sum(((cosPulse(60e-9) >> (t0 + 5e-9)) for t0 in starts[1:]), cosPulse(60e-9) >> (starts[0] + 5e-9)) * 0.5
        chans += [i_row, q_row]
    gates = BatchSampler(chans, ('linspace', 0.0, n / rate, n, False)).launch_torch(
        torch.empty((2 * pairs, n), dtype=torch.float64, device=dev()))
    dac = distortion.DacStage.from_full_scale(1.0, n, batch=2 * pairs, bits=14, shift=2, interleave=2)
    pair_codes = dac.apply_torch(gates)
    mk = distortion.MarkerStage(n, lead=lead, trail=trail, group=2, batch=2 * pairs)
    mk.apply_codes_torch(gates, pair_codes, bit=0)
    seg = distortion.SegmentStage(n, batch=pairs, width=2, align=16)
    table, packed, used = seg.apply_torch(pair_codes, bit=0)
    codes = pair_codes.cpu().numpy()
    want = ref.library_ref(table.cpu().numpy(), packed.cpu().numpy(), used.cpu().numpy(), 2)
    segments = seg.download(table, packed, used)
    for bits in ALL_BITS:
        lib = distortion.SegmentLibrary.of(seg)
        with hash_bits(bits):
            out = lib.apply_torch(table, packed, used)                      # (the plan is made here)
        assert lib.kernel_name(0) == 'seglib_hash' + ('' if bits is None else f' [hash bits {bits}]')
        rows_out = lib.download(*out, used)
        same(out[3].cpu().numpy(), want[3], f'end to end, bits {bits}: lib_used')
        for g, (p, s, y) in enumerate(rows_out):
            same(p, want[0][g], f'end to end, bits {bits}: plays of pair {g}')
            same(s, want[1][g], f'end to end, bits {bits}: slots of pair {g}')
            same(y, want[2][g], f'end to end, bits {bits}: library of pair {g}')
            idle = codes[g, :2]
            back = distortion.expand_segments(p, y, n, idle, width=2)
            assert np.array_equal(back, distortion.expand_segments(*segments[g], n, idle, width=2))
            assert np.array_equal(back, codes[g]) and len(p) == len(starts) and len(y) <= len(segments[g][1])
        lib.close()
    for s in (dac, mk, seg):
        s.close()


@pytest.mark.parametrize('k', [1, 2])
def test_codes_tiled_from_three_shapes_give_three_slots(k):
    """a dedupe case with a known answer: rows tiled on the device from 3 pulse shapes (the marker in bit 0, idle
    between them), cut by the segment stage, give unique == 3 and a library of the three pulses"""
    align, period, rows, plays_per_row = 16, 256, 4, 60
    n = period * plays_per_row
    g = torch.Generator(device='cpu').manual_seed(160 + k)
    lengths = (48, 80, 112)                                                      # multiples of the granule
    pulses = [(torch.randint(-32768, 32768, (k * L,), generator=g, dtype=torch.int32) | 1).to(torch.int16).to(dev())
              for L in lengths]
    codes = torch.zeros((rows, k * n), dtype=torch.int16, device=dev())
    order = torch.randint(0, 3, (rows, plays_per_row), generator=g)
    order[:, :3] = torch.tensor([0, 1, 2])
    for r in range(rows):
        for j in range(plays_per_row):
            d = int(order[r, j])
            at = k * (period * j + 32)                                           # every pulse on the same granule phase
            codes[r, at:at + k * lengths[d]] = pulses[d]
    seg = distortion.SegmentStage(n, batch=rows, width=k, align=align)
    table, packed, used = seg.apply_torch(codes, bit=0)
    for bits in ALL_BITS:
        lib = distortion.SegmentLibrary.of(seg)
        with hash_bits(bits):
            plays, slots, library, lib_used = lib.apply_torch(table, packed, used)   # (the plan is made here)
        assert lib.kernel_name(1) == 'seglib_match' + ('' if bits is None else f' [hash bits {bits}]')
        assert lib_used.cpu().numpy().tolist() == [[3, sum(lengths)]] * rows
        assert used.cpu().numpy()[:, 0].tolist() == [plays_per_row] * rows
        same(slots.cpu().numpy()[:, :plays_per_row], order.numpy().astype(np.int32), f'tiled: slots, bits {bits}')
        want = torch.cat(pulses).cpu().numpy()
        for r in range(rows):
            same(library[r, :k * sum(lengths)].cpu().numpy(), want, f'tiled: library of row {r}, bits {bits}')
            p, _, y = lib.download(plays, slots, library, lib_used, used)[r]
            assert np.array_equal(distortion.expand_segments(p, y, n, 0, width=k), codes[r].cpu().numpy())
        lib.close()
    seg.close()


def test_plain_c_consumer_builds_the_library_on_the_device(tmp_path):
    exe = tmp_path / 'segment_library_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'segment_library_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    for bits in ALL_BITS:
        env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
        env.pop('WFK_SEGLIB_HASH_BITS', None)
        if bits is not None:
            env['WFK_SEGLIB_HASH_BITS'] = str(bits)
        r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (bits, r.returncode, r.stdout, r.stderr)
        assert 'library on the device, parity ok' in r.stdout, (bits, r.stdout)


def test_a_value_that_is_no_number_of_bits_is_ignored():
    """include/wfk.h: WFK_SEGLIB_HASH_BITS outside [0, 64] or no whole number leaves the full hash, and the names say so"""
    for value in ('', 'x', '-1', '65', '4 ', '0x4', '1.5'):
        lib = distortion.SegmentLibrary(1, 4, 16)
        with hash_bits(value):
            assert [lib.kernel_name(i) for i in range(2)] == ['seglib_hash', 'seglib_match'], value
        lib.close()
    lib = distortion.SegmentLibrary(1, 4, 16)
    with hash_bits(64):
        assert lib.kernel_name(0) == 'seglib_hash'
    lib.close()
