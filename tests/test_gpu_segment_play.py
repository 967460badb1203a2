"""The segment player on the device (distortion.SegmentPlayer / play_rows, csrc/wfk_segment_play.hip) against the
referee tests/segment_play_ref.py, the NumPy statement of the semantics.  Codes and counts are integers: every
comparison here is exact.  Every apply goes through `check`, which gives the player windows of wider sentinel-filled
tensors at given leads (the wide rows a multiple of 16 bytes apart, so every row of a case has the lead's phase) and
compares the WHOLE of them with what the referee says -- the codes the player owes, and the sentinel everywhere else:
every gap of a strided row and every code of a bad row -- fills the report with garbage first, compares the inputs as
bits afterwards, applies a second time, and runs the verifying pass (into nothing: a sentinel-filled out stays as it
is) and the checking pass.  The cases that do not go through `check` (streams, graph replay, far rows, the large
case, play_rows, the refusals, the chains, the C consumer) say so."""
import os
import subprocess

import numpy as np
import pytest
import torch

import graph_replay
import segment_play_ref as ref
from row_windows import FarWindow, bits_equal, free_far_arena
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO, SY, SE = -23101, 0x7a7a, 0x1b1b          # what out holds before an apply; around the packed and the expect windows
GARBAGE = 0x5a5a5a5a5a
S = 8192                                     # wfk_segment_play_span; test_span_and_names holds it to the library


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}; last at {tuple(bad[-1])}')


def wide_codes(values, lead, fill):
    """host (rows, m) int16 -> (the wide device tensor, rows a multiple of 8 codes apart, filled with `fill`; its
    window of m codes `lead` codes in, holding `values`)"""
    rows, m = values.shape
    width = -(-(m + 16) // 8) * 8
    wide = torch.full((rows, width), fill, dtype=torch.int16, device=dev())
    win = wide[:, lead:lead + m]
    win.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    return wide, win


def check(table, packed, used, n, k=1, idle=0, expect=None, what='', out_lead=3, packed_lead=5, expect_lead=1,
          table_lead=1, capacity=None):
    """a player for the case, windows at the given leads (codes; ints for the table), the play twice, play + verify,
    the verifying pass and the checking pass against the referee; the inputs compared as bits afterwards
    -> (out (rows, k n), report) of the referee (with `expect` where it is given)"""
    rows, ms = table.shape[0], table.shape[1]
    cap = packed.shape[1] // k if capacity is None else capacity
    wide_t = torch.full((rows, 3 * ms + 8), -1, dtype=torch.int32, device=dev())
    tw = wide_t.as_strided((rows, ms, 3), (wide_t.stride(0), 3, 1), table_lead)
    tw.copy_(torch.from_numpy(table))
    wide_y, yw = wide_codes(packed[:, :k * cap], packed_lead, SY)
    ud = torch.from_numpy(used).to(dev())
    inputs, names = [wide_t, wide_y, ud], ['table', 'packed', 'used']
    ew = None
    if expect is not None:
        wide_e, ew = wide_codes(expect[:, :k * n], expect_lead, SE)
        inputs.append(wide_e), names.append('expect')
    before = [x.cpu().numpy().copy() for x in inputs]
    want_out, want_plain = ref.expected_out(table, packed, used, n, idle, k, SO, cap)
    _, want_report = ref.expected_out(table, packed, used, n, idle, k, SO, cap, expect)
    blank = np.full((rows, k * n), SO, dtype=np.int16)
    player = distortion.SegmentPlayer(n, rows, k, ms, cap)
    try:
        def fresh(values):
            return wide_codes(values, out_lead, SO)

        full = fresh(want_out)[0].cpu().numpy()
        wide_o, ow = fresh(blank)
        report = torch.full((rows, 4), GARBAGE, dtype=torch.int64, device=dev())
        for turn in ('first apply', 'second apply'):
            o, r = player.apply_torch(tw, yw, ud, idle=idle, out=ow, report=report)
            assert (o.data_ptr(), r.data_ptr()) == (ow.data_ptr(), report.data_ptr()) and tuple(o.shape) == (rows, k * n)
            same(report.cpu().numpy(), want_plain, f'{what}: report of the play, {turn}')
            same(wide_o.cpu().numpy(), full, f'{what}: out, {turn}')
            report.fill_(-GARBAGE)
        if expect is not None:
            wide_o, ow = fresh(blank)
            player.apply_torch(tw, yw, ud, idle=idle, out=ow, expect=ew, report=report)
            same(report.cpu().numpy(), want_report, f'{what}: report of play + verify')
            same(wide_o.cpu().numpy(), full, f'{what}: out of play + verify')
            wide_o, ow = fresh(blank)
            for turn in ('first', 'second'):
                report.fill_(GARBAGE)
                assert player.verify_torch(tw, yw, ud, ew, idle=idle, report=report) is report
                same(report.cpu().numpy(), want_report, f'{what}: report of the verifying pass, {turn}')
            same(player.verify_torch(tw, yw, ud, ew, idle=idle).cpu().numpy(), want_report, f'{what}: verify, allocated')
            same(wide_o.cpu().numpy(), fresh(blank)[0].cpu().numpy(), f'{what}: an out that no apply was given')
        report.fill_(GARBAGE)
        same(player.check_torch(tw, yw, ud, report=report).cpu().numpy(), want_plain, f'{what}: checking pass')
        same(player.check_torch(tw, yw, ud).cpu().numpy(), want_plain, f'{what}: checking pass, allocated')
        o, r = player.apply_torch(tw, yw, ud, idle=idle)                       # both allocated
        good = want_plain[:, 0] >= 0
        same(o.cpu().numpy()[good], want_out[good], f'{what}: out, allocated')
        same(r.cpu().numpy(), want_plain, f'{what}: report, allocated')
        for x, b, name in zip(inputs, before, names):
            assert bits_equal(x.cpu().numpy(), b), f'{what}: {name} was written'
    finally:
        player.close()
    return want_out, want_report


def planted(want_out, report, k, n, seed, count=5):
    """`want_out` with a code changed at the first and the last code of every good row and at `count` random codes"""
    e = want_out.copy()
    rng = np.random.default_rng(seed)
    for r in range(len(e)):
        if report[r, 0] < 0 or n == 0:
            e[r] = SE
            continue
        at = {0, k * n - 1} | set(rng.integers(0, k * n, count).tolist())
        for c in at:
            e[r, c] ^= np.int16(1 << int(rng.integers(0, 15)))
    return e


def geometry_rows(n, k, seed):
    """no plays, one play over the whole row, bursts, every other sample a one-sample play, bursts in packed order"""
    whole = (np.array([[0, n, 2]], dtype=np.int32), np.arange(k * (n + 2)).astype(np.int16), n + 2)
    return [(np.zeros((0, 3), np.int32), np.zeros(0, np.int16), 0), whole, ref.random_table(n, k, seed, lead=3),
            ref.random_table(n, k, seed + 1, dense=True), ref.random_table(n, k, seed + 2, lead=0, shuffle_offsets=False)]


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('n', [1, 2, 7, 8, 9, 63, 64, 65, 255, 257, S - 1, S, S + 1, 2 * S + 1, 10007])
def test_geometry(n, k):
    rows = geometry_rows(n, k, 7 * n + k)
    table, packed, used = ref.stack_rows(rows, k, max_segments=max(len(r[0]) for r in rows) + 1)
    assert used[3, 0] == (n + 1) // 2 and (n < 600 or used[3, 0] > 256)              # more than one tile of entries
    idle = [-7, 9][:k]
    want_out, report = ref.expected_out(table, packed, used, n, idle, k, SO)
    assert np.all(report[:, 0] >= 0) and report[1, 0] == n
    check(table, packed, used, n, k, idle, planted(want_out, report, k, n, n), what=f'n={n} k={k}',
          out_lead=0 if n % 2 else 3, expect_lead=n % 8)


@pytest.mark.parametrize('k', [1, 2])
def test_plays_across_block_edges(k):
    n = 3 * S + 100
    t = np.array([[3, 5, 1], [S - 5, S + 10, 20],                # from block 0 into block 2
                  [2 * S + 5, S - 5, 7], [3 * S, 7, 0],          # ends at a block edge, the next starts there
                  [3 * S + 50, 1, 9], [n - 1, 1, 2 * S]],        # the row's last sample
                 dtype=np.int32)
    rng = np.random.default_rng(5)
    packed = rng.integers(-32768, 32768, k * (2 * S + 40)).astype(np.int16)
    table, pk, used = ref.stack_rows([(t, packed, 2 * S + 40), (t[1:4], packed, 2 * S + 40)], k)
    for lead in (0, 1):
        want_out, report = ref.expected_out(table, pk, used, n, 0, k, SO)
        assert report[:, 0].tolist() == [int(t[:, 1].sum()), int(t[1:4, 1].sum())]
        e = planted(want_out, report, k, n, 11)
        for c in (k * (S - 5), k * S, k * (2 * S + 4), k * (2 * S + 5), k * 3 * S - 1, k * 3 * S, k * (3 * S + 7)):
            e[:, c] ^= 0x40
        check(table, pk, used, n, k, 0, e, what=f'block edges k={k} lead {lead}', out_lead=lead, packed_lead=lead)


def phases_case(k):
    """64 plays: starts of every residue mod 8 against offsets of every residue mod 8, lengths that end anywhere"""
    t, off = [], 0
    for a in range(8):
        for b in range(8):
            j = 8 * a + b
            off = (off + 7) // 8 * 8 + b
            length = 17 + (5 * j) % 23
            t.append([48 * j + a, length, off])
            off += length
    t = np.asarray(t, dtype=np.int32)
    rng = np.random.default_rng(20 + k)
    return t, rng.integers(-32768, 32768, k * off).astype(np.int16), off, 48 * 64 + 11


@pytest.mark.parametrize('k', [1, 2])
def test_every_lead_and_every_source_phase(k):
    t, packed, cap, n = phases_case(k)
    assert sorted({(int(s) % 8, int(o) % 8) for s, _, o in t}) == [(a, b) for a in range(8) for b in range(8)]
    user = t.copy()
    user[:, 2] |= 1                                               # a user's table: every offset odd (k = 2: 4 bytes + 2)
    user = user[(user[:, 2] + user[:, 1]) <= cap]
    table, pk, used = ref.stack_rows([(t, packed, cap), (user, packed, cap), (t[::3], packed, cap)], k)
    idle = [3, -4][:k]                                            # two idle codes: I on I positions whatever the lead
    want_out, report = ref.expected_out(table, pk, used, n, idle, k, SO)
    e = planted(want_out, report, k, n, 30 + k, count=40)
    for lead in range(8):
        check(table, pk, used, n, k, idle, e, what=f'out lead {lead} k={k}', out_lead=lead, packed_lead=0, expect_lead=0)
        check(table, pk, used, n, k, idle, e, what=f'packed lead {lead} k={k}', out_lead=0, packed_lead=lead, expect_lead=0)
        check(table, pk, used, n, k, idle, e, what=f'expect lead {lead} k={k}', out_lead=0, packed_lead=0, expect_lead=lead)
        check(table, pk, used, n, k, idle, e, what=f'all leads {lead} k={k}', out_lead=lead, packed_lead=(3 * lead + 1) % 8,
              expect_lead=(5 * lead + 2) % 8, table_lead=lead % 4)


def tiled_codes(k, rows=3, plays_per_row=40, period=256):
    """rows tiled on the device from 3 pulse shapes with the marker in bit 0, idle (0) between them"""
    n = period * plays_per_row
    g = torch.Generator(device='cpu').manual_seed(160 + k)
    lengths = (48, 80, 112)
    pulses = [(torch.randint(-32768, 32768, (k * L,), generator=g, dtype=torch.int32) | 1).to(torch.int16) for L in lengths]
    codes = torch.zeros((rows, k * n), dtype=torch.int16)
    order = torch.randint(0, 3, (rows, plays_per_row), generator=g)
    for r in range(rows):
        for j in range(plays_per_row):
            d = int(order[r, j])
            at = k * (period * j + 37 + r)                                   # pulses on no granule's edge
            codes[r, at:at + k * lengths[d]] = pulses[d]
    return codes.to(dev()), n


@pytest.mark.parametrize('align', [1, 16, 64])
@pytest.mark.parametrize('k', [1, 2])
def test_the_stage_and_the_library_as_sources(k, align):
    codes, n = tiled_codes(k)
    rows = codes.shape[0]
    seg = distortion.SegmentStage(n, batch=rows, width=k, align=align)
    table, packed, used = seg.apply_torch(codes, bit=0)
    player = distortion.SegmentPlayer.of(seg)
    out, report = player.apply_torch(table, packed, used, idle=0, expect=codes)
    host = codes.cpu().numpy()
    same(out.cpu().numpy(), host, f'the stage as the source, align {align}')   # the codes under the marker, idle elsewhere
    kept = used.cpu().numpy()[:, 1]
    same(report.cpu().numpy(), np.stack([kept, 0 * kept, 0 * kept, 0 * kept - 1], axis=1), 'its report')
    want, _ = ref.play_ref(table.cpu().numpy(), packed.cpu().numpy(), used.cpu().numpy(), n, 0, k)
    same(out.cpu().numpy(), np.stack(want), 'the stage as the source against the referee')
    lib = distortion.SegmentLibrary.of(seg)
    plays, slots, library, lib_used = lib.apply_torch(table, packed, used)
    assert lib_used.cpu().numpy()[:, 0].tolist() == [3] * rows               # three shapes, forty plays
    of_lib = distortion.SegmentPlayer.of(lib, n)
    out2, report2 = of_lib.apply_torch(plays, library, used, idle=0, expect=codes)
    same(report2.cpu().numpy(), report.cpu().numpy(), 'the library as the source: report')
    assert bits_equal(out2.cpu().numpy(), out.cpu().numpy()), 'the two outs differ'
    # an idle code that the rows do not hold: stray = the samples outside the plays that are not 77 -- all of them
    r3 = of_lib.verify_torch(plays, library, used, codes, idle=77).cpu().numpy()
    assert r3[:, 1].tolist() == [0] * rows and (r3[:, 2] == n - kept).all() and (r3[:, 3] >= 0).all()
    for x in (seg, player, lib, of_lib):
        x.close()


@pytest.mark.parametrize('k', [1, 2])
def test_report_on_planted_differences(k):
    n = 3 * S + 77
    t = np.array([[5, 4, 3], [9, 3, 20], [20, 11, 8], [40, 1, 0], [S + 100, 300, 31], [2 * S + 9, S, 400]], dtype=np.int32)
    rng = np.random.default_rng(40 + k)
    packed = rng.integers(-32768, 32768, k * (S + 400)).astype(np.int16)
    table, pk, used = ref.stack_rows([(t, packed, S + 400)], k)
    idle = [-1, -2][:k]
    want_out, report = ref.expected_out(table, pk, used, n, idle, k, SO)
    played = int(t[:, 1].sum())

    def run(*codes, want):
        e = want_out.copy()
        for c in set(codes):
            e[0, c] ^= 0x10
        got = check(table, pk, used, n, k, idle, e, what=f'planted {codes} k={k}', out_lead=0, expect_lead=len(codes) % 8)[1]
        assert got.tolist() == [[played] + want], (codes, got)

    run(want=[0, 0, -1])                                                      # expect = what is played
    run(k * 5, want=[1, 0, 5])                                                # the first code of a play
    run(k * 31 - 1, want=[1, 0, 30])                                          # the last code of a play
    run(k * 2, want=[0, 1, 2])                                                # before the first play
    run(k * 15, want=[0, 1, 15])                                              # in the first gap
    run(k * n - 1, want=[0, 1, n - 1])                                        # in the last gap: the row's last code
    run(k * 8, k * 9, k * 12, want=[2, 1, 8])
    run(k * (2 * S + 500), k * (S + 3), k * 25, want=[2, 1, 25])              # one in each of three blocks: first by the
    run(k * (2 * S + 500), k * (S + 3), want=[1, 1, S + 3])                   # atomic min, whichever block arrives first
    run(k * (3 * S + 70), k * (S + 200), k * 100, k * (2 * S + 8), want=[1, 3, 100])
    if k == 2:
        run(2 * 22 + 1, want=[1, 0, 22])                                      # the second code of a pair only
        run(2 * 22 + 1, 2 * 22, 2 * 17 + 1, want=[1, 1, 17])
    player = distortion.SegmentPlayer(n, 1, k, len(t), S + 400)
    td, yd, ud = (torch.from_numpy(x).to(dev()) for x in (table, pk, used))
    out, _ = player.apply_torch(td, yd, ud, idle=idle)
    assert player.verify_torch(td, yd, ud, out, idle=idle).cpu().numpy().tolist() == [[played, 0, 0, -1]]
    player.close()


BAD = (('count -1', lambda t, u, n, cap, ms: u.__setitem__((1, 0), -1)),
       ('count max_segments + 1', lambda t, u, n, cap, ms: u.__setitem__((1, 0), ms + 1)),
       ('count 2^40', lambda t, u, n, cap, ms: u.__setitem__((1, 0), 2**40)),
       ('length 0', lambda t, u, n, cap, ms: t.__setitem__((1, 2, 1), 0)),
       ('length -1', lambda t, u, n, cap, ms: t.__setitem__((1, 2, 1), -1)),
       ('a negative start', lambda t, u, n, cap, ms: t.__setitem__((1, 0, 0), -1)),
       ('start + length = n + 1', lambda t, u, n, cap, ms: t.__setitem__((1, 4), [n - 4, 5, 0])),
       ('a negative offset', lambda t, u, n, cap, ms: t.__setitem__((1, 3, 2), -1)),
       ('offset + length = capacity + 1', lambda t, u, n, cap, ms: t.__setitem__((1, 4), [n - 5, 5, cap - 4])),
       ('overlapping by one sample', lambda t, u, n, cap, ms: t.__setitem__((1, 3, 0), t[1, 2, 0] + t[1, 2, 1] - 1)),
       ('not ascending', lambda t, u, n, cap, ms: t.__setitem__((1, 3), [0, 1, 0])),
       ('2^31 - 1', lambda t, u, n, cap, ms: t.__setitem__((1, 4), [2**31 - 1, 2**31 - 1, 2**31 - 1])))


@pytest.mark.parametrize('k', [1, 2])
def test_a_bad_row_is_reported_and_left_alone(k):
    n, cap, ms = S + 300, 600, 5

    def rows_of():
        t = np.array([[10, 100, 7], [110, 50, 200], [300, 64, 300], [S - 3, 9, 400], [S + 100, 100, 500]], dtype=np.int32)
        rng = np.random.default_rng(50 + k)
        return ref.stack_rows([(t, rng.integers(-32768, 32768, k * cap).astype(np.int16), cap)] * 3, k)

    table, packed, used = rows_of()
    want_out, report = check(table, packed, used, n, k, 5, what=f'three good rows k={k}')
    assert (report[:, 0] == 323).all()
    table[1, 1] = [110, 190, 0]                                               # touching on both sides: good
    table[1, 4] = [n - 5, 5, cap - 5]                                         # to the ends of the row and of the room
    assert check(table, packed, used, n, k, 5, what=f'touching k={k}')[1][1, 0] == 100 + 190 + 64 + 9 + 5
    for name, spoil in BAD:
        table, packed, used = rows_of()
        spoil(table, used, n, cap, ms)
        e = planted(want_out, report, k, n, 60)
        got_out, got = check(table, packed, used, n, k, 5, e, what=f'{name} k={k}', out_lead=0)
        assert got[1].tolist() == [-1] * 4 and (got[[0, 2], 0] == 323).all() and (got[[0, 2], 3] == 0).all(), (name, got)
        assert (got_out[1] == SO).all() and np.array_equal(got_out[[0, 2]], want_out[[0, 2]])
    # an overflowed stage: used holds the true count, above max_segments
    codes = torch.zeros((3, k * n), dtype=torch.int16, device=dev())
    codes.view(3, n, k)[:, ::16, 0] = 1                                       # every 16th sample a segment
    codes.view(3, n, k)[2, 16 * 40:] = 0                                      # row 2 fits: 40 segments
    seg = distortion.SegmentStage(n, batch=3, width=k, align=1, max_segments=40, capacity=n)
    t, p, u = seg.apply_torch(codes, bit=0)
    player = distortion.SegmentPlayer.of(seg)
    out = torch.full((3, k * n), SO, dtype=torch.int16, device=dev())
    _, r = player.apply_torch(t, p, u, out=out, expect=codes)
    assert u.cpu().numpy()[:, 0].tolist() == [-(-n // 16), -(-n // 16), 40]
    assert r.cpu().numpy().tolist() == [[-1] * 4, [-1] * 4, [40, 0, 0, -1]]
    got = out.cpu().numpy()
    assert (got[:2] == SO).all() and np.array_equal(got[2], codes[2].cpu().numpy())
    player.close()
    seg.close()


def test_an_overlap_at_the_edges_of_the_rounds_of_the_check():
    """the neighbour condition where the entry before sits in another round of 64, or in the rounds before"""
    k, n = 1, 2300
    good = ref.random_table(n, k, 65, dense=True)                              # 1150 one-sample plays, 2 apart
    for j in (1, 63, 64, 65, 127, 128, 192, 255, 256, 257, 320, 511, 512, 960, 1023, 1024, 1025, 1088, 1149):
        touching, overlapping = good[0].copy(), good[0].copy()
        touching[j, 0] -= 1                                                    # starts where the one before ends: good
        overlapping[j, 0] -= 2                                                 # on the one before: bad
        table, packed, used = ref.stack_rows([good, (touching,) + good[1:], (overlapping,) + good[1:]], k)
        got = check(table, packed, used, n, k, 3, what=f'entry {j} on the one before')[1]
        assert got.tolist() == [[1150, 0, 0, -1], [1150, 0, 0, -1], [-1] * 4], (j, got)


def test_span_and_names():
    for k in (1, 2):
        player = distortion.SegmentPlayer(100, 2, k, 4, 50)
        assert player.span() == S == distortion.SegmentStage(100, align=1).span()
        assert [player.kernel_name(i) for i in range(5)] == [
            'segplay_check', f'segplay_fill<{k}, true, false>', f'segplay_fill<{k}, false, true>',
            f'segplay_fill<{k}, true, true>', '']
        player.close()


def plumbing_case(k, rows, n, seed):
    made = [ref.random_table(n, k, seed + i, lead=i % 4) for i in range(rows)]
    table, packed, used = ref.stack_rows(made, k)
    return table, packed, used


def test_side_stream_equals_default_stream():
    k, rows, n = 2, 3, 2 * S + 33
    table, packed, used = plumbing_case(k, rows, n, 70)
    want_out, _ = ref.expected_out(table, packed, used, n, [1, 2], k, SO)
    expect = planted(want_out, np.zeros((rows, 4)), k, n, 71)
    _, want_report = ref.expected_out(table, packed, used, n, [1, 2], k, SO, expect=expect)
    player = distortion.SegmentPlayer(n, rows, k, table.shape[1], packed.shape[1] // k)
    outs = []
    side = torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), side):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            td, yd, ud, ed = (torch.from_numpy(x).to(dev()) for x in (table, packed, used, expect))
            got = player.apply_torch(td, yd, ud, idle=[1, 2], expect=ed)
            outs.append(tuple(x + 0 for x in got))                           # produced and consumed on that stream
        stream.synchronize()
    for name, (o, r) in zip(('default', 'side'), outs):
        same(o.cpu().numpy(), want_out, f'{name} stream: out')
        same(r.cpu().numpy(), want_report, f'{name} stream: report')
    player.close()


def test_graph_replay_on_other_inputs():
    k, rows, n, ms, cap = 2, 3, S + 501, 700, 6000
    feeds = []
    for seed in (80, 81, 82):
        made = [ref.random_table(n, k, seed + 10 * i, lead=i) for i in range(rows)]
        assert all(len(m[0]) <= ms and m[2] <= cap for m in made)
        table, packed, used = ref.stack_rows(made, k, max_segments=ms, capacity=cap)
        if seed == 81:
            table[1, 4, 0] = table[1, 3, 0]                                  # a row that turns bad, and good again
        out, report = ref.expected_out(table, packed, used, n, [4, -4], k, 0)
        feeds.append([table, packed, used, planted(out, report, k, n, seed)])
    player = distortion.SegmentPlayer(n, rows, k, ms, cap)
    td = torch.empty((rows, ms, 3), dtype=torch.int32, device=dev())
    yd = torch.empty((rows, k * cap), dtype=torch.int16, device=dev())
    ud = torch.empty((rows, 2), dtype=torch.int64, device=dev())
    ed = torch.empty((rows, k * n), dtype=torch.int16, device=dev())
    out = torch.empty((rows, k * n), dtype=torch.int16, device=dev())
    report = torch.empty((rows, 4), dtype=torch.int64, device=dev())
    verdict = torch.empty((rows, 4), dtype=torch.int64, device=dev())

    def run():
        player.apply_torch(td, yd, ud, idle=[4, -4], out=out, expect=ed, report=report)
        player.verify_torch(td, yd, ud, ed, idle=[4, -4], report=verdict)

    got = graph_replay.replay(run, [td, yd, ud, ed], feeds, [out, report, verdict])
    bad = []
    for turn, ((o, r, v), (table, packed, used, expect)) in enumerate(zip(got, feeds)):
        want_out, want_report = ref.expected_out(table, packed, used, n, [4, -4], k, SO, expect=expect)
        same(r, want_report, f'replay {turn}: report')
        same(v, want_report, f'replay {turn}: report of the verifying pass')
        same(o, want_out, f'replay {turn}: out')                             # (the helper's sentinel for int16 is SO)
        bad.append(want_report[1].tolist() == [-1] * 4)
        assert (want_report[[0, 2], 3] == 0).all()
    assert bad == [False, True, False]
    player.close()


def test_far_rows():
    """out rows more than 2^32 codes apart: the played codes as the referee has them, every guard of the arena untouched"""
    k, n = 1, 2**17 - 3
    made = [ref.random_table(n, k, 90 + i, lead=1 + i) for i in range(2)]
    table, packed, used = ref.stack_rows(made, k)
    want_out, want_report = ref.expected_out(table, packed, used, n, -9, k, SO)
    expect = planted(want_out, want_report, k, n, 91)
    _, want_verdict = ref.expected_out(table, packed, used, n, -9, k, SO, expect=expect)
    try:
        far = FarWindow(n, np.int16)
        td, yd, ud, ed = (torch.from_numpy(x).to(dev()) for x in (table, packed, used, expect))
        player = distortion.SegmentPlayer(n, 2, k, table.shape[1], packed.shape[1] // k)
        try:
            o, r = player.apply_torch(td, yd, ud, idle=-9, out=far.win, expect=ed)
            same(r.cpu().numpy(), want_verdict, 'far out rows: report')
            same(far.host(), want_out, 'far out rows: out')
            far.assert_guards()
        finally:
            player.close()
        del far, o
    finally:
        free_far_arena()


def test_sixty_four_rows_of_100003():
    k, rows, n = 1, 64, 100003
    made = [ref.random_table(n, k, 100 + i, lead=i % 8) for i in range(4)]
    made += [ref.random_table(n, k, 104, dense=True)]
    table, packed, used = ref.stack_rows([made[i % 5] for i in range(rows)], k)
    want_out, want_plain = ref.expected_out(table[:5], packed[:5], used[:5], n, 21, k, SO)
    want_out, want_plain = want_out[np.arange(rows) % 5], want_plain[np.arange(rows) % 5]
    expect = want_out.copy()
    expect[:, ::997] ^= 2
    inside = np.stack([ref.play_row_searchsorted(table[i], packed[i], used[i, 0], n, 21, k)[1] for i in range(5)])
    hit = np.zeros(n, dtype=bool)
    hit[::997] = True
    td, yd, ud, ed = (torch.from_numpy(x).to(dev()) for x in (table, packed, used, expect))
    player = distortion.SegmentPlayer(n, rows, k, table.shape[1], packed.shape[1] // k)
    out, report = player.apply_torch(td, yd, ud, idle=21, expect=ed)
    same(out.cpu().numpy(), want_out, '64 x 100003: out')
    want = want_plain.copy()
    for r in range(rows):
        want[r, 1:] = [(inside[r % 5] & hit).sum(), (~inside[r % 5] & hit).sum(), 0]
    same(report.cpu().numpy(), want, '64 x 100003: report')
    player.close()


def test_play_rows_against_the_referee():
    for k in (1, 2):
        n = S + 19
        made = [ref.random_table(n, k, 110 + i, lead=i) for i in range(3)] + [(np.zeros((0, 3), np.int32), np.zeros(0, np.int16), 0)]
        segments = [(m[0], m[1]) for m in made]
        table, packed, used = ref.stack_rows(made, k)
        idle = [6, -6][:k]
        want_out, want_plain = ref.expected_out(table, packed, used, n, idle, k, SO)
        same(distortion.play_rows(segments, n, idle=idle, width=k), want_out, f'play_rows k={k}')
        expect = planted(want_out, want_plain, k, n, 111)
        _, want_report = ref.expected_out(table, packed, used, n, idle, k, SO, expect=expect)
        out, report = distortion.play_rows(segments, n, idle=idle, width=k, expect=expect, return_report=True)
        same(out, want_out, f'play_rows with expect k={k}')
        same(report, want_report, f'play_rows: report k={k}')
        for r in range(3):
            same(out[r], distortion.expand_segments(*segments[r], n, idle, width=k), f'play_rows against expand_segments, row {r}')
        broken = (made[1][0].copy(), made[1][1])
        broken[0][1, 0] = broken[0][0, 0]                                     # overlapping: expand_segments takes it
        with pytest.raises(ValueError, match='play_rows: row 1: the table cannot be played'):
            distortion.play_rows([segments[0], broken], n, width=k)
        out0 = distortion.play_rows([(made[0][0][:0], made[0][1])], 0, width=k, return_report=True)
        assert out0[0].shape == (1, 0) and out0[1].tolist() == [[0, 0, 0, -1]]


def test_refused_tensors():
    rows, k, n, ms, cap = 2, 2, 16, 6, 64
    player = distortion.SegmentPlayer(n, rows, k, ms, cap)
    table = torch.zeros((rows, ms, 3), dtype=torch.int32, device=dev())
    packed = torch.zeros((rows, k * cap), dtype=torch.int16, device=dev())
    used = torch.zeros((rows, 2), dtype=torch.int64, device=dev())
    out = torch.full((rows, k * n), 9, dtype=torch.int16, device=dev())
    expect = torch.zeros((rows, k * n), dtype=torch.int16, device=dev())
    report = torch.full((rows, 4), 5, dtype=torch.int64, device=dev())
    player.apply_torch(table, packed, used, out=out, expect=expect, report=report)   # fine
    torch.cuda.synchronize()
    assert report.cpu().numpy().tolist() == [[0, 0, 0, -1]] * rows and not out.cpu().numpy().any()
    report.fill_(5), out.fill_(9)
    A, V, K = player.apply_torch, player.verify_torch, player.check_torch
    for bad in (table[:1], table[:, :ms - 1], table.to(torch.int64), table.cpu(), table.view(rows, 3 * ms),
                table.permute(0, 2, 1).contiguous().permute(0, 2, 1)):
        for call in (lambda: A(bad, packed, used), lambda: V(bad, packed, used, expect), lambda: K(bad, packed, used)):
            with pytest.raises(ValueError, match='expected table'):
                call()
    for bad in (packed[:1], packed[:, :k * cap - 1], packed.to(torch.int32), packed.cpu(), packed.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected packed'):
            A(table, bad, used)
    for bad in (out[:1], out[:, :k * n - 1], out.to(torch.int32), out.cpu(), out.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected out'):
            A(table, packed, used, out=bad)
        with pytest.raises(ValueError, match='expected expect'):
            A(table, packed, used, expect=bad)
        with pytest.raises(ValueError, match='expected expect'):
            V(table, packed, used, bad)
    with pytest.raises(ValueError, match='expected expect'):
        V(table, packed, used, None)
    for bad in (used[:1], used.view(-1), used.to(torch.int32), used.cpu(), None,
                torch.zeros((rows, 3), dtype=torch.int64, device=dev())[:, :2]):
        with pytest.raises(ValueError, match='expected used'):
            A(table, packed, bad)
    for bad in (report[:1], report.view(-1), report.to(torch.int32), report.cpu(),
                torch.zeros((rows, 5), dtype=torch.int64, device=dev())[:, :4]):
        for call in (lambda: A(table, packed, used, report=bad), lambda: V(table, packed, used, expect, report=bad),
                     lambda: K(table, packed, used, report=bad)):
            with pytest.raises(ValueError, match='expected report'):
                call()
    for idle, message in (([1, 2, 3], 'idle is one code'), (1.5, 'idle must be a whole number'), (2**15, 'idle must lie in')):
        with pytest.raises(ValueError, match='segment play: ' + message):
            A(table, packed, used, idle=idle)
        with pytest.raises(ValueError, match='segment play: ' + message):
            V(table, packed, used, expect, idle=idle)
    as_report = packed.view(-1)[8:8 + 16 * rows].view(torch.int64).view(rows, 4)
    for kw, message in ((dict(out=packed[:, :k * n]), 'out overlaps packed'), (dict(out=expect, expect=expect), 'out overlaps expect'),
                        (dict(out=table.view(torch.int16).view(rows, -1)[:, :k * n]), 'out overlaps table'),
                        (dict(report=as_report), 'report overlaps'),
                        (dict(report=out.view(-1)[:16 * rows].view(torch.int64).view(rows, 4), out=out), 'report overlaps'),
                        (dict(report=expect.view(-1)[:16 * rows].view(torch.int64).view(rows, 4), expect=expect), 'report overlaps')):
        with pytest.raises(ValueError, match=message):
            A(table, packed, used, **kw)
    with pytest.raises(ValueError, match='report overlaps'):
        V(table, packed, used, expect, report=as_report)
    with pytest.raises(ValueError, match='report overlaps'):
        K(table, packed, used, report=as_report)
    torch.cuda.synchronize()
    assert np.all(report.cpu().numpy() == 5) and np.all(out.cpu().numpy() == 9)
    player.close()
    empty = distortion.SegmentPlayer(0, rows, k, 0, 0)                               # nothing to hold: the report alone
    o, r = empty.apply_torch(table[:, :0], packed[:, :0], used, expect=expect[:, :0])
    assert tuple(o.shape) == (rows, 0) and r.cpu().numpy().tolist() == [[0, 0, 0, -1]] * rows
    used2 = used.clone()
    used2[1, 0] = 1                                                                  # an entry where there is room for none
    assert empty.check_torch(table[:, :0], packed[:, :0], used2).cpu().numpy().tolist() == [[0, 0, 0, -1], [-1] * 4]
    empty.close()


def test_library_refuses_a_bad_apply():
    """the C side's own checks of an apply, through the raw pointers; nothing is launched"""
    rows, k, n, ms, cap = 2, 1, 40, 6, 64
    player = distortion.SegmentPlayer(n, rows, k, ms, cap)
    table = torch.zeros((rows, ms, 3), dtype=torch.int32, device=dev())
    packed = torch.zeros((rows, cap), dtype=torch.int16, device=dev())
    used = torch.zeros((rows, 2), dtype=torch.int64, device=dev())
    out = torch.full((rows, n), 9, dtype=torch.int16, device=dev())
    expect = torch.zeros((rows, n), dtype=torch.int16, device=dev())
    report = torch.full((rows, 4), 5, dtype=torch.int64, device=dev())
    t, y, u, o, e, r = (x.data_ptr() for x in (table, packed, used, out, expect, report))
    plan, i = player._plan(), (0, 0)
    plan.apply(t, 3 * ms, y, cap, u, i, o, n, e, n, r)                              # fine
    torch.cuda.synchronize()
    assert report.cpu().numpy().tolist() == [[0, 0, 0, -1]] * rows and not out.cpu().numpy().any()
    report.fill_(5), out.fill_(9)
    for args, message in (((t, 3 * ms, y, cap, u, i, o, n, e, n, None), 'report is null'),
                          ((t, 3 * ms, y, cap, None, i, o, n, e, n, r), 'used is null'),
                          ((None, 3 * ms, y, cap, u, i, o, n, e, n, r), 'null'),
                          ((t, 3 * ms, None, cap, u, i, None, 0, None, 0, r), 'null'),
                          ((t, 3 * ms - 1, y, cap, u, i, o, n, e, n, r), 'table row stride smaller'),
                          ((t, 3 * ms, y, cap - 1, u, i, o, n, e, n, r), 'packed row stride smaller'),
                          ((t, 3 * ms, y, cap, u, i, o, n - 1, e, n, r), 'out row stride smaller'),
                          ((t, 3 * ms, y, cap, u, i, o, n, e, n - 1, r), 'expect row stride smaller'),
                          ((t, 3 * ms, y, cap, u, i, None, 0, e, n - 1, r), 'expect row stride smaller'),
                          ((t + 2, 3 * ms, y, cap, u, i, o, n, e, n, r), 'not aligned'),
                          ((t, 3 * ms, y + 1, cap, u, i, o, n, e, n, r), 'not aligned'),
                          ((t, 3 * ms, y, cap, u + 4, i, o, n, e, n, r), 'not aligned'),
                          ((t, 3 * ms, y, cap, u, i, o + 1, n, e, n, r), 'not aligned'),
                          ((t, 3 * ms, y, cap, u, i, o, n, e + 1, n, r), 'not aligned'),
                          ((t, 3 * ms, y, cap, u, i, o, n, e, n, r + 4), 'counts are not aligned'),
                          ((t, 3 * ms, y, cap, u, i, y + 2, n, e, n, r), 'out overlaps packed'),
                          ((t, 3 * ms, y, cap, u, i, t + 4, n, e, n, r), 'out overlaps table'),
                          ((t, 3 * ms, y, cap, u, i, u, n, e, n, r), 'out overlaps used'),
                          ((t, 3 * ms, y, cap, u, i, e + 2, n, e, n, r), 'out overlaps expect'),
                          ((t, 3 * ms, y, cap, u, i, o, n, e, n, u), 'counts overlaps used'),
                          ((t, 3 * ms, y, cap, u, i, o, n, e, n, o + 8), 'counts overlaps out'),
                          ((t, 3 * ms, y, cap, u, i, None, 0, e, n, e + 8), 'counts overlaps expect'),
                          ((t, 3 * ms, y, cap, u, i, None, 0, None, 0, y + 8), 'counts overlaps packed'),
                          ((t, 3 * ms - 1, y, cap, u, i, None, 0, None, 0, r), 'table row stride smaller')):
        with pytest.raises(_engine.EngineError, match=message):
            plan.apply(*args)
    torch.cuda.synchronize()
    assert np.all(report.cpu().numpy() == 5) and np.all(out.cpu().numpy() == 9)
    player.close()


def test_end_to_end_gates_to_played_rows():
    """the README chain: I/Q pairs of pulses sampled at 2 GS/s -> 14-bit codes with the switch marker in bit 0 -> cut in
    granules of 16 samples -> the library -> the player: the device-side check of the upload (differ == 0, stray = what
    the cut dropped: nothing here, the rows are the ideal gates) and the played rows fed to a Demodulator"""
    from waveforms_amd import cosPulse, gaussian
    from waveforms_amd._sampling import BatchSampler
    from waveforms_amd.utils import Demodulator
    n, rate, pairs = 8000, 2e9, 3
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
    mk = distortion.MarkerStage(n, lead=20, trail=10, group=2, batch=2 * pairs)
    mk.apply_codes_torch(gates, pair_codes, bit=0)
    seg = distortion.SegmentStage(n, batch=pairs, width=2, align=16)
    table, packed, used = seg.apply_torch(pair_codes, bit=0)
    lib = distortion.SegmentLibrary.of(seg)
    plays, slots, library, lib_used = lib.apply_torch(table, packed, used)
    codes = pair_codes.cpu().numpy()
    idle = codes[0, :2]
    kept = used.cpu().numpy()[:, 1]
    for player, t, y in ((distortion.SegmentPlayer.of(seg), table, packed), (distortion.SegmentPlayer.of(lib, n), plays, library)):
        played, report = player.apply_torch(t, y, used, idle=idle, expect=pair_codes)
        same(report.cpu().numpy(), np.stack([kept, 0 * kept, 0 * kept, 0 * kept - 1], axis=1), 'end to end: report')
        same(played.cpu().numpy(), codes, 'end to end: the played rows')
        dm = Demodulator([50e6, 125e6], 2 * n, dtype=np.int16)
        assert np.array_equal(dm.apply_torch(played).cpu().numpy(), dm.apply_torch(pair_codes).cpu().numpy())
        # a predistorted row never returns to idle: what the cut drops is counted, not lost from sight
        tail = pair_codes.clone()
        tail[:, -100:] += 4
        stray = player.verify_torch(t, y, used, tail, idle=idle).cpu().numpy()
        assert stray[:, 1].tolist() == [0] * pairs and stray[:, 2].tolist() == [50] * pairs and stray[:, 3].tolist() == [n - 50] * pairs
        player.close()
    for s in (dac, mk, seg, lib):
        s.close()


def test_plain_c_consumer_plays_on_the_device(tmp_path):
    exe = tmp_path / 'segment_play_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'segment_play_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'played on the device, parity ok' in r.stdout, r.stdout
