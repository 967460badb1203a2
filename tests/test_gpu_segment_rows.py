"""The segment stage on the device (distortion.SegmentStage / segment_rows, csrc/wfk_segment_rows.hip) against the
referee tests/segment_rows_ref.py, the NumPy statement of the semantics.  Tables, packed codes and totals are integers:
every comparison here is exact.  Every apply goes through `check`, which gives the stage windows of wider
sentinel-filled tensors and compares the WHOLE of them with what the referee says: the entries and codes the stage
owes, and the sentinel everywhere else -- beyond a truncated table, beyond the kept codes, around and between strided
rows.  Sizes follow the kernel's real geometry through `.span()`."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import graph_replay
import marker_rows_ref
import segment_rows_ref as ref
from row_windows import FarWindow, bits_equal, free_far_arena
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 255, 257, 'S-1', 'S', 'S+1', '2S+1', 10007]
ALIGNS = (1, 8, 64)
FORMS = (('bit', 0), ('bit', 15), ('marks', None))
ST, SP = 0x5EC7AB1E, -23101                    # what the table and the packed rows hold before an apply
GARBAGE = 0x5a5a5a5a5a


def dev():
    return torch.device('cuda', torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def span(align=1):
    st = distortion.SegmentStage(8, align=align)
    try:
        return st.span()
    finally:
        st.close()


def size_of(size, S):
    return size if isinstance(size, int) else {'S-1': S - 1, 'S': S, 'S+1': S + 1, '2S+1': 2 * S + 1}[size]


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}; last at {tuple(bad[-1])}')


def inputs(m, k, form, seed, one_code_only=True):
    """mask (rows, n) -> (codes, bit, marks) of a form: the bit form carries the mask in one bit of random codes (on one
    code of a pair only), the marks form in bytes next to codes whose every bit is random"""
    kind, bit = form
    if kind == 'bit':
        return ref.codes_with(m, k, bit, seed, one_code_only=one_code_only), bit, None
    rng = np.random.default_rng(seed)
    codes = rng.integers(-32768, 32768, (m.shape[0], k * m.shape[1])).astype(np.int16)
    return codes, None, (m * rng.integers(1, 256, m.shape)).astype(np.uint8)


def expected(codes, k, align, bit, marks, max_segments, capacity):
    """-> (table (rows, max_segments, 3) and packed (rows, k capacity) as an apply leaves sentinel-filled ones, used,
    the referee's per-row tables and packed codes)"""
    tables, packed, used = ref.segment_ref(codes, k, align, bit=bit, marks=marks)
    rows = codes.shape[0]
    T = np.full((rows, max_segments, 3), ST, dtype=np.int32)
    P = np.full((rows, k * capacity), SP, dtype=np.int16)
    for g in range(rows):
        c, q = min(len(tables[g]), max_segments), k * min(int(used[g, 1]), capacity)
        T[g, :c] = tables[g][:c]
        P[g, :q] = packed[g][:q]
    return T, P, used, tables, packed


def check(codes, k=1, align=1, bit=None, marks=None, max_segments=None, capacity=None, what='', code_lead=3,
          packed_lead=5, marks_lead=1, stage=None):
    """one stage, windows at the given leads (elements) into wider tensors, two applies and the sizing pass against the
    referee; the inputs compared as bits afterwards -> (used, tables, packed) of the referee"""
    rows, n = codes.shape[0], codes.shape[1] // k
    st = stage or distortion.SegmentStage(n, rows, k, align, max_segments, capacity)
    try:
        ms, cap = st.max_segments, st.capacity
        wide_c = torch.full((rows, k * n + 24), -1, dtype=torch.int16, device=dev())      # every bit set around the rows
        cw = wide_c[:, code_lead:code_lead + k * n]
        cw.copy_(torch.from_numpy(codes))
        wide_m = mw = None
        if marks is not None:
            wide_m = torch.full((rows, n + 40), 1, dtype=torch.uint8, device=dev())
            mw = wide_m[:, marks_lead:marks_lead + n]
            mw.copy_(torch.from_numpy(marks))
        before = wide_c.cpu().numpy().copy(), (wide_m.cpu().numpy().copy() if marks is not None else None)
        wide_t = torch.full((rows, ms + 3, 3), ST, dtype=torch.int32, device=dev())
        wide_p = torch.full((rows, k * cap + 24), SP, dtype=torch.int16, device=dev())
        tw, pw = wide_t[:, 1:1 + ms], wide_p[:, packed_lead:packed_lead + k * cap]
        used = torch.full((rows, 2), GARBAGE, dtype=torch.int64, device=dev())
        want_t, want_p, want_used, tables, packed = expected(codes, k, align, bit, marks, ms, cap)
        full_t = np.full((rows, ms + 3, 3), ST, dtype=np.int32)
        full_t[:, 1:1 + ms] = want_t
        full_p = np.full((rows, k * cap + 24), SP, dtype=np.int16)
        full_p[:, packed_lead:packed_lead + k * cap] = want_p
        for turn in ('first apply', 'second apply'):
            t, p, u = st.apply_torch(cw, bit=bit, marks=mw, table=tw, packed=pw, used=used)
            assert t.data_ptr() == tw.data_ptr() and p.data_ptr() == pw.data_ptr() and u.data_ptr() == used.data_ptr()
            assert tuple(t.shape) == (rows, ms, 3) and tuple(p.shape) == (rows, k * cap)
            same(used.cpu().numpy(), want_used, f'{what}: used, {turn}')
            same(wide_t.cpu().numpy(), full_t, f'{what}: table, {turn}')
            same(wide_p.cpu().numpy(), full_p, f'{what}: packed, {turn}')
            used.fill_(-GARBAGE)
        same(st.measure_torch(cw, bit=bit, marks=mw, used=used).cpu().numpy(), want_used, f'{what}: sizing pass')
        same(st.measure_torch(cw, bit=bit, marks=mw).cpu().numpy(), want_used, f'{what}: sizing pass, allocated')
        assert bits_equal(wide_c.cpu().numpy(), before[0]), f'{what}: the codes were written'
        assert marks is None or bits_equal(wide_m.cpu().numpy(), before[1]), f'{what}: the marks were written'
        same(wide_t.cpu().numpy(), full_t, f'{what}: table after the sizing pass')
        return want_used, tables, packed
    finally:
        if stage is None:
            st.close()


@pytest.mark.parametrize('size', SIZES)
def test_shapes(size):
    S = span()
    assert S == 8192
    n = size_of(size, S)
    for align in ALIGNS:
        for k in (1, 2):
            for form in FORMS:
                masks = (ref.bursts_mask(3, n, n + align + k, gate=max(align, 5)), ref.alternate_mask(3, n, align, phase=k - 1))
                for which, m in enumerate(masks):
                    codes, bit, marks = inputs(m, k, form, 7 * n + which)
                    what = f'n={n} A={align} k={k} {form} mask {which}'
                    used, _, _ = check(codes, k, align, bit, marks, what=what)
                    if which == 1 and k == 1 and n >= 2 * align:                  # the most segments a row can have
                        assert used[0, 0] == (-(-n // align) + 1) // 2, what


def test_stage_reports_its_geometry():
    for k in (1, 2):
        st = distortion.SegmentStage(100, batch=2, width=k, align=16)
        assert st.plan is None and st.span() == 8192 and st.plan is not None
        assert [st.kernel_name(i) for i in range(3)] == [f'segment_count<{k}, false>', 'segment_scan',
                                                         f'segment_pack<{k}, false>']
        assert st.kernel_name(2, marks=True) == f'segment_pack<{k}, true>' and st.kernel_name(3) == ''
        st.close()
        assert st.plan is None
    assert span(64) == span(128) == 8192 and span(256) == 16384 and span(4096) == 262144


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('align', [1, 8, 64, 256, 4096])
def test_masks_at_the_block_edges(align, k):
    S = span(align)
    n = 3 * S + 11
    form = FORMS[(k + align) % 3]
    rows = []
    m = np.zeros((2, n), dtype=bool)                       # all off, all on
    m[1] = True
    rows.append(('off / on', m))
    m = np.zeros((6, n), dtype=bool)                       # one sample either side of a block edge
    for r, (s, d) in enumerate((s, d) for s in (1, 2) for d in (-1, 0, 1)):
        m[r, s * S + d] = True
    rows.append(('single samples', m))
    m = np.zeros((2, n), dtype=bool)                       # from block 0 into block 2: block 1 has no edge in it
    m[0, S // 2:2 * S + S // 2] = True
    m[1, S - 1:2 * S + 1] = True
    rows.append(('across a whole block', m))
    m = np.zeros((3, n), dtype=bool)                       # ends at a block edge, the next starts there + A
    m[0, S - 3 * align:S] = True
    m[0, S + align:S + 2 * align] = True
    m[1, :S] = True                                        # the whole first block, then the whole last stretch
    m[1, 2 * S:] = True
    m[2, 2 * S - 1] = True                                 # ends at an edge; the next block starts kept
    m[2, 2 * S] = True
    rows.append(('at the edge', m))
    rows.append(('every other granule', ref.alternate_mask(2, n, align)))
    for name, m in rows:
        codes, bit, marks = inputs(m, k, form, 3 * align + k)
        used, tables, _ = check(codes, k, align, bit, marks, what=f'{name} A={align} k={k} {form}')
        if name == 'across a whole block':
            assert used[:, 0].tolist() == [1, 1] and tables[0][0, 1] >= 2 * S
        if name == 'at the edge':
            assert tables[0].tolist() == [[S - 3 * align, 3 * align, 0], [S + align, align, 3 * align]]
            assert tables[1].tolist() == [[0, S, 0], [2 * S, S + 11, S]] and used[2].tolist() == [1, 2 * align]
        if name == 'single samples':
            assert used.tolist() == [[1, align]] * 6


@pytest.mark.parametrize('k', [1, 2])
def test_truncation_is_by_position_and_reports_the_true_totals(k):
    S = span()
    n, align = 2 * S + 300, 8
    m = ref.bursts_mask(3, n, 31, gate=60)
    m[2] = False
    m[2, 100:S + 40] = True                                # a segment across the block edge: kept - 1 cuts it in block 1,
    m[2, S + 500:S + 600] = True                           # kept // 2 in mid-block 0
    for form in FORMS[1:]:
        codes, bit, marks = inputs(m, k, form, 32)
        _, _, used = ref.segment_ref(codes, k, align, bit=bit, marks=marks)
        count, kept = int(used[:, 0].max()), int(used[:, 1].max())
        assert count > 3 and used[2].tolist() == [2, S - 56 + 104]
        for ms in (0, count - 1, count, 1):
            for cap in (0, kept - 1, kept, int(used[2, 1]) - 1, int(used[2, 1]) // 2 + 3, 5):
                got, _, _ = check(codes, k, align, bit, marks, ms, cap, what=f'max_segments={ms} capacity={cap} k={k} {form}')
                assert np.array_equal(got, used)


@pytest.mark.parametrize('k', [1, 2])
def test_every_alignment_of_the_rows(k):
    n = 1000 + k
    for align in (1, 4, 16):
        m = ref.bursts_mask(3, n, 40 + align, gate=20)
        for lead in range(16):
            form = FORMS[lead % 3]
            codes, bit, marks = inputs(m, k, form, lead)
            check(codes, k, align, bit, marks, code_lead=lead % 8, packed_lead=(lead // 2 + lead) % 8, marks_lead=lead,
                  what=f'leads {lead} A={align} k={k} {form}')
    codes, bit, marks = inputs(m, k, FORMS[0], 50)
    for code_lead in range(8):                             # and every pair of code and packed leads at A k >= 8
        for packed_lead in range(8):
            check(codes, k, 16, bit, marks, code_lead=code_lead, packed_lead=packed_lead,
                  what=f'code lead {code_lead} packed lead {packed_lead} k={k}')


def test_row_independence():
    n, align = 10007, 8
    m = ref.bursts_mask(5, n, 60, gate=30)
    codes, bit, marks = inputs(m, 1, FORMS[0], 61)
    alone = ref.segment_ref(codes[:1], 1, align, bit=bit)
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [1, 0, 2]):
        _, tables, packed = check(codes[order], 1, align, bit, what=f'rows {order}')
        at = order.index(0)
        assert np.array_equal(tables[at], alone[0][0]) and np.array_equal(packed[at], alone[1][0])


def test_side_stream_equals_default_stream():
    n, rows, k, align = 3 * span() + 5, 3, 2, 16
    m = ref.bursts_mask(rows, n, 70, gate=100)
    codes, bit, _ = inputs(m, k, FORMS[0], 71)
    want_t, want_p, want_used, _, _ = expected(codes, k, align, bit, None, (-(-n // align) + 1) // 2, n)
    st = distortion.SegmentStage(n, rows, k, align)
    outs = []
    side = torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), side):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            cd = torch.from_numpy(codes).to(dev())
            table = torch.full((rows, st.max_segments, 3), ST, dtype=torch.int32, device=dev())
            packed = torch.full((rows, k * n), SP, dtype=torch.int16, device=dev())
            t, p, u = st.apply_torch(cd, bit=bit, table=table, packed=packed)
            outs.append((t + 0, p + 0, u + 0))             # produced and consumed on that stream
        stream.synchronize()
    for name, (t, p, u) in zip(('default', 'side'), outs):
        same(t.cpu().numpy(), want_t, f'{name} stream, table')
        same(p.cpu().numpy(), want_p, f'{name} stream, packed')
        same(u.cpu().numpy(), want_used, f'{name} stream, used')
    st.close()


@pytest.mark.parametrize('form', ['bit', 'marks'])
def test_graph_replay_on_other_codes(form):
    n, rows, k, align = 2 * span() + 77, 3, 2, 16
    st = distortion.SegmentStage(n, rows, k, align, max_segments=40, capacity=n // 2)
    feeds, wants = [], []
    for seed, duty in ((80, 0.2), (81, 0.05), (82, 0.6)):
        m = ref.bursts_mask(rows, n, seed, duty=duty, gate=90)
        codes, bit, marks = inputs(m, k, FORMS[0] if form == 'bit' else FORMS[2], seed)
        feeds.append([codes] if form == 'bit' else [codes, marks])
        wants.append(expected(codes, k, align, bit, marks, 40, n // 2)[:3])
    cd = torch.empty((rows, k * n), dtype=torch.int16, device=dev())
    md = torch.empty((rows, n), dtype=torch.uint8, device=dev())
    table = torch.empty((rows, 40, 3), dtype=torch.int32, device=dev())
    packed = torch.empty((rows, k * (n // 2)), dtype=torch.int16, device=dev())
    used = torch.empty((rows, 2), dtype=torch.int64, device=dev())

    def run():
        if form == 'bit':
            st.apply_torch(cd, bit=0, table=table, packed=packed, used=used)
        else:
            st.apply_torch(cd, marks=md, table=table, packed=packed, used=used)

    got = graph_replay.replay(run, [cd] if form == 'bit' else [cd, md], feeds, [table, packed, used])
    sent_t, sent_p = graph_replay._sentinel_of(4), graph_replay._sentinel_of(2)
    overflowed = 0
    for turn, ((t, p, u), (want_t, want_p, want_used)) in enumerate(zip(got, wants)):
        want_t, want_p = want_t.copy(), want_p.copy()
        want_t[want_t == ST] = sent_t                       # (the helper's sentinels, not this file's)
        untouched = np.arange(want_p.shape[1])[None, :] >= k * np.minimum(want_used[:, 1:2], n // 2)
        want_p[untouched] = sent_p
        same(u, want_used, f'replay {turn} {form}: used')
        same(t, want_t, f'replay {turn} {form}: table')
        same(p, want_p, f'replay {turn} {form}: packed')
        overflowed += int((want_used[:, 1] > n // 2).sum())
    assert overflowed and len({tuple(w[2].reshape(-1)) for w in wants}) == 3
    st.close()


def test_far_rows():
    """code rows more than 2^32 codes apart: the table, the packed codes and the totals as the referee has them, every
    guard of the arena untouched, the codes bit for bit what was put there"""
    n, align = 2**17 - 3, 16
    m = ref.bursts_mask(2, n, 90, gate=200)
    codes, bit, _ = inputs(m, 1, FORMS[0], 91)
    st = distortion.SegmentStage(n, 2, 1, align)
    want_t, want_p, want_used, _, _ = expected(codes, 1, align, bit, None, st.max_segments, n)
    assert want_used[:, 0].min() > 20
    try:
        src = FarWindow(n, np.int16, codes)
        table = torch.full((2, st.max_segments, 3), ST, dtype=torch.int32, device=dev())
        packed = torch.full((2, n), SP, dtype=torch.int16, device=dev())
        _, _, used = st.apply_torch(src.win, bit=bit, table=table, packed=packed)
        same(used.cpu().numpy(), want_used, 'far codes: used')
        same(table.cpu().numpy(), want_t, 'far codes: table')
        same(packed.cpu().numpy(), want_p, 'far codes: packed')
        src.assert_holds(codes)
        del src
    finally:
        st.close()
        free_far_arena()


@pytest.mark.parametrize('k,form', [(1, FORMS[2]), (2, FORMS[0])])
def test_many_workgroups_per_row(k, form):
    rows, n, align = 64, 100003, 16
    m = ref.bursts_mask(rows, n, 100, gate=256)
    codes, bit, marks = inputs(m, k, form, 101)
    used, _, _ = check(codes, k, align, bit, marks, what=f'{rows} x {n} k={k} {form}', code_lead=0, packed_lead=0,
                       marks_lead=0)
    assert used[:, 0].min() >= 10 and len({tuple(u) for u in used.tolist()}) > rows // 2
    assert 0.1 < used[:, 1].sum() / (rows * n) < 0.4


def test_download_returns_the_rows_and_raises_on_an_overflow():
    n, rows, k, align = 9000, 4, 2, 16
    m = ref.bursts_mask(rows, n, 110, gate=80)
    m[3] = False                                            # a row that keeps nothing
    codes, bit, _ = inputs(m, k, FORMS[0], 111)
    tables, packed, used = ref.segment_ref(codes, k, align, bit=bit)
    cd = torch.from_numpy(codes).to(dev())
    st = distortion.SegmentStage(n, rows, k, align)
    got = st.download(*st.apply_torch(cd, bit=bit))
    assert len(got) == rows and used[3].tolist() == [0, 0]
    for g, (t, p) in enumerate(got):
        same(t, tables[g], f'download: table of row {g}')
        same(p, packed[g], f'download: packed of row {g}')
        back = distortion.expand_segments(t, p, n, 0, width=k)
        on = np.repeat(m[g], k)
        assert np.array_equal(back[on], codes[g][on])
    st.close()
    count, kept = int(used[:, 0].max()), int(used[:, 1].max())
    for kw, message in ((dict(max_segments=count - 1), 'overflowed'), (dict(capacity=kept - 1), 'overflowed')):
        tight = distortion.SegmentStage(n, rows, k, align, **kw)
        out = tight.apply_torch(cd, bit=bit)
        with pytest.raises(ValueError, match=f'row {int(used[:, 0].argmax()) if "max_segments" in kw else int(used[:, 1].argmax())} {message}'):
            tight.download(*out)
        tight.close()
    exact = distortion.SegmentStage(n, rows, k, align, max_segments=count, capacity=kept)
    for (t, p), wt, wp in zip(exact.download(*exact.apply_torch(cd, bit=bit)), tables, packed):
        same(t, wt, 'download at the exact sizes: table')
        same(p, wp, 'download at the exact sizes: packed')
    exact.close()
    got = distortion.segment_rows(codes, bit=bit, width=k, align=align)        # NumPy in, NumPy out
    marked = distortion.segment_rows(codes, marks=m, width=k, align=align)
    for g in range(rows):
        for t, p in (got[g], marked[g]):
            same(t, tables[g], f'segment_rows: table of row {g}')
            same(p, packed[g], f'segment_rows: packed of row {g}')


def test_refused_tensors():
    n, rows, k = 256, 2, 2
    st = distortion.SegmentStage(n, rows, k, 8)
    ms = st.max_segments
    codes = torch.zeros((rows, k * n), dtype=torch.int16, device=dev())
    marks = torch.zeros((rows, n), dtype=torch.uint8, device=dev())
    table = torch.zeros((rows, ms, 3), dtype=torch.int32, device=dev())
    packed = torch.zeros((rows, k * n), dtype=torch.int16, device=dev())
    used = torch.zeros((rows, 2), dtype=torch.int64, device=dev())
    st.apply_torch(codes, bit=0, table=table, packed=packed, used=used)        # fine
    st.apply_torch(codes, marks=marks, table=table, packed=packed, used=used)
    for kw in (dict(), dict(bit=0, marks=marks)):
        with pytest.raises(ValueError, match='exactly one'):
            st.apply_torch(codes, **kw)
        with pytest.raises(ValueError, match='exactly one'):
            st.measure_torch(codes, **kw)
    for bit in (-1, 16):
        with pytest.raises(ValueError, match='bit'):
            st.apply_torch(codes, bit=bit)
    for bad in (codes[:1], codes[:, :k * n - 1], codes.to(torch.int32), codes.cpu(), codes.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected codes'):
            st.apply_torch(bad, bit=0)
        with pytest.raises(ValueError, match='expected codes'):
            st.measure_torch(bad, bit=0)
    for bad in (marks[:1], marks[:, :n - 1], marks.to(torch.int16), marks.cpu(), marks.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected marks'):
            st.apply_torch(codes, marks=bad)
    for bad in (table[:1], table[:, :ms - 1], table.to(torch.int64), table.cpu(), table.view(rows, 3 * ms),
                table.permute(0, 2, 1).contiguous().permute(0, 2, 1)):
        with pytest.raises(ValueError, match='expected table'):
            st.apply_torch(codes, bit=0, table=bad)
    for bad in (packed[:1], packed[:, :k * n - 1], packed.to(torch.int32), packed.cpu(), packed.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected packed'):
            st.apply_torch(codes, bit=0, packed=bad)
    for bad in (used[:1], used.view(-1), used.to(torch.int32), used.cpu(), torch.zeros((rows, 3), dtype=torch.int64, device=dev())[:, :2]):
        with pytest.raises(ValueError, match='expected used'):
            st.apply_torch(codes, bit=0, used=bad)
        with pytest.raises(ValueError, match='expected used'):
            st.measure_torch(codes, bit=0, used=bad)
    as_table = codes.view(-1)[:rows * ms * 6].view(torch.int32).view(rows, ms, 3)
    as_used = packed.view(-1)[8:8 + 8 * rows].view(torch.int64).view(rows, 2)
    for kw, message in ((dict(packed=codes), 'packed overlaps codes'), (dict(table=as_table), 'table overlaps codes'),
                        (dict(table=as_table, marks=marks), 'table overlaps codes'),
                        (dict(packed=marks.view(torch.int16).view(1, -1).expand(rows, -1), marks=marks), 'expected packed'),
                        (dict(table=marks.view(torch.int32)[:, :3 * ms].view(rows, ms, 3), marks=marks), 'table overlaps marks'),
                        (dict(table=packed.view(-1)[:rows * ms * 6].view(torch.int32).view(rows, ms, 3), packed=packed),
                         'table overlaps packed'),
                        (dict(used=as_used, packed=packed), 'used overlaps'),
                        (dict(used=codes.view(-1)[:8 * rows].view(torch.int64).view(rows, 2)), 'used overlaps')):
        kw = dict(dict(bit=0) if 'marks' not in kw else {}, **kw)
        with pytest.raises(ValueError, match=message):
            st.apply_torch(codes, **kw)
    with pytest.raises(ValueError, match='used overlaps'):
        st.measure_torch(codes, bit=0, used=codes.view(-1)[:8 * rows].view(torch.int64).view(rows, 2))
    torch.cuda.synchronize()
    assert not table.cpu().numpy().any() and not packed.cpu().numpy().any() and not used.cpu().numpy().any()
    st.close()
    empty = distortion.SegmentStage(0, rows, k, 8)                             # n = 0: used zeroed, nothing else
    used.fill_(7)
    t, p, u = empty.apply_torch(torch.zeros((rows, 0), dtype=torch.int16, device=dev()), bit=3, used=used)
    assert tuple(t.shape) == (rows, 0, 3) and tuple(p.shape) == (rows, 0) and not u.cpu().numpy().any()
    assert empty.download(t, p, u)[1][0].shape == (0, 3)
    empty.close()


def test_library_refuses_a_bad_apply():
    """the C side's own checks of an apply, through the raw pointers; nothing is launched"""
    n, rows, k = 64, 2, 1
    st = distortion.SegmentStage(n, rows, k, 8)
    ms = st.max_segments
    codes = torch.zeros((rows, n), dtype=torch.int16, device=dev())
    marks = torch.zeros((rows, n), dtype=torch.uint8, device=dev())
    table = torch.zeros((rows, ms, 3), dtype=torch.int32, device=dev())
    packed = torch.zeros((rows, n), dtype=torch.int16, device=dev())
    used = torch.full((rows, 2), 5, dtype=torch.int64, device=dev())
    c, m, t, p, u = (x.data_ptr() for x in (codes, marks, table, packed, used))
    plan = st._plan()
    plan.apply_bit(c, n, 0, t, 3 * ms, p, n, u)                                # fine
    plan.apply_marks(c, n, m, n, t, 3 * ms, p, n, u)
    torch.cuda.synchronize()
    assert not used.cpu().numpy().any()
    used.fill_(5)
    lib = _engine.lib()
    for bit in (-1, 16):
        assert lib.wfk_segment_rows_apply_bit(plan._h, c, n, bit, t, 3 * ms, p, n, u, None) == -1
        assert b'bit must lie in [0, 15]' in lib.wfk_last_error()
    for args, message in (((c, n, 0, t, 3 * ms, p, n, None), 'used is null'),
                          ((c, n, 0, None, 0, p, n, u), 'null table with a packed'),
                          ((c, n, 0, t, 3 * ms, None, 0, u), 'null packed with a table'),
                          ((None, n, 0, t, 3 * ms, p, n, u), 'null'),
                          ((c, n - 1, 0, t, 3 * ms, p, n, u), 'codes row stride smaller'),
                          ((c, n, 0, t, 3 * ms - 1, p, n, u), 'table row stride smaller'),
                          ((c, n, 0, t, 3 * ms, p, n - 1, u), 'packed row stride smaller'),
                          ((c + 1, n, 0, t, 3 * ms, p, n, u), 'not aligned'),
                          ((c, n, 0, t + 2, 3 * ms, p, n, u), 'not aligned'),
                          ((c, n, 0, t, 3 * ms, p + 1, n, u), 'not aligned'),
                          ((c, n, 0, t, 3 * ms, p, n, u + 4), 'counts are not aligned'),
                          ((c, n, 0, t, 3 * ms, c + 2, n, u), 'packed overlaps codes'),
                          ((c, n, 0, c + 4, 3 * ms, p, n, u), 'table overlaps codes'),
                          ((c, n, 0, p + 4, 3 * ms, p, n, u), 'table overlaps packed'),
                          ((c, n, 0, t, 3 * ms, p, n, c + 8), 'counts overlaps codes'),
                          ((c, n, 0, t, 3 * ms, p, n, t + 8), 'counts overlaps table'),
                          ((c, n, 0, None, 0, None, 0, c + 8), 'counts overlaps codes'),
                          ((c, n - 1, 0, None, 0, None, 0, u), 'codes row stride smaller')):
        with pytest.raises(_engine.EngineError, match=message):
            plan.apply_bit(*args)
    for args, message in (((c, n, None, n, t, 3 * ms, p, n, u), 'null marks'),
                          ((c, n, m, n - 1, t, 3 * ms, p, n, u), 'marks row stride smaller'),
                          ((c, n, m, n, t, 3 * ms, m, n, u), 'packed overlaps marks'),
                          ((c, n, m, n, m, 3 * ms, p, n, u), 'table overlaps marks'),
                          ((c, n, m, n, t, 3 * ms, p, n, m + 8), 'counts overlaps marks')):
        with pytest.raises(_engine.EngineError, match=message):
            plan.apply_marks(*args)
    torch.cuda.synchronize()
    assert np.all(used.cpu().numpy() == 5) and not table.cpu().numpy().any() and not packed.cpu().numpy().any()
    st.close()
    empty = distortion.SegmentStage(0, rows, k, 8)                             # n = 0: null rows, used zeroed
    h = empty._plan()._h
    assert lib.wfk_segment_rows_apply_bit(h, None, 0, 0, None, 0, None, 0, u, None) == 0
    assert lib.wfk_segment_rows_apply_marks(h, None, 0, None, 0, None, 0, None, 0, u, None) == 0
    torch.cuda.synchronize()
    assert not used.cpu().numpy().any()
    assert lib.wfk_segment_rows_apply_bit(h, None, 0, 0, None, 0, None, 0, u + 4, None) == -1
    assert b'counts are not aligned' in lib.wfk_last_error()
    empty.close()


def test_end_to_end_gates_to_segments():
    """the README chain: I/Q pairs of gaussian / cosPulse pulses sampled on a 2 GS/s grid -> 14-bit codes, interleaved,
    left-justified -> the switch marker of each pair in bit 0 -> cut in granules of 16 samples -> downloaded ->
    expanded with the pair's idle code: the codes again wherever the marker is set, one segment per pulse"""
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
    counts = torch.empty((pairs, 2), dtype=torch.int64, device=dev())
    mk.apply_codes_torch(gates, pair_codes, bit=0, counts=counts)
    seg = distortion.SegmentStage(n, batch=pairs, width=2, align=16)
    table, packed, used = seg.apply_torch(pair_codes, bit=0)
    segments = seg.download(table, packed, used)
    codes = pair_codes.cpu().numpy()
    want_m, want_counts = marker_rows_ref.marker_ref(gates.cpu().numpy(), lead, trail, 0.0, 2)
    tables, packs, want_used = ref.segment_ref(codes, 2, 16, bit=0)
    same(used.cpu().numpy(), want_used, 'end to end: used')
    assert used.cpu().numpy()[:, 0].tolist() == want_counts[:, 1].tolist() == [len(starts)] * pairs
    assert np.array_equal(want_m, (codes[:, ::2] & 1) | (codes[:, 1::2] & 1))
    for g, (t, p) in enumerate(segments):
        same(t, tables[g], f'end to end: table of pair {g}')
        same(p, packs[g], f'end to end: packed of pair {g}')
        idle = codes[g, :2]                                 # the pair's code of 0.0: the row starts idle
        assert not want_m[g, 0] and not np.any(idle & 1)
        back = distortion.expand_segments(t, p, n, idle, width=2)
        on = np.repeat(want_m[g].astype(bool), 2)
        assert np.array_equal(back[on], codes[g][on])
        assert np.array_equal(back, codes[g])               # and idle everywhere else: the gates are exact zeros there
        assert len(p) < codes.shape[1] // 2                 # what crosses to the host
    for s in (dac, mk, seg):
        s.close()


def test_plain_c_consumer_cuts_on_the_device(tmp_path):
    exe = tmp_path / 'segment_rows_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'segment_rows_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'cut on the device, parity ok' in r.stdout, r.stdout
