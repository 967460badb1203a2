"""The fused mix-to-codes stage on the device (distortion.MixDacStage / mix_dac_rows, csrc/wfk_mix_dac.hip) against BOTH
the NumPy referee (tests/mix_dac_ref.py: dac_ref(mix_ref(...))) and the two stages it replaces, MixStage followed by
DacStage, on the same device.  Codes and counts are integers and every rounding of the formula is stated: every
comparison here is for equality, there is no tolerance anywhere."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import dac_rows_ref
import graph_replay
import mix_dac_ref as ref
import mix_rows_ref as mref
from row_windows import FarWindow, Window, free_far_arena
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _engine.MIX_DAC_TILE_ROWS
NP_OF = {'f64': np.float64, 'f32': np.float32}
TORCH_OF = {'f64': torch.float64, 'f32': torch.float32}
NAME_OF = {'f64': 'double', 'f32': 'float'}
SPAN = 4096                                              # kSlots * kThreads * 4 samples: one workgroup's span of a mix row
SIZES = [1, 2, 7, 8, 9, 15, 16, 17, SPAN - 1, SPAN, SPAN + 1, 10007]
FORMATS = [(16, 0), (14, 2), (2, 14)]                    # (bits, shift)
SENTINEL = -21846                                        # 0xAAAA


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def gains_offsets(rows, bits):
    """gains of both signs around 0.8 hi per unit of the MIXED signal (the inputs lie in [-1, 1] and the matrices add a
    few of them up: rows clip on both rails), fractional offsets of both signs"""
    hi = 2**(bits - 1) - 1
    g = np.array([0.8, -0.8, 0.5, -0.37, 1.0, 0.93])[np.arange(rows) % 6] * hi
    o = np.array([0.0, 12.5, -300.25, 0.5, hi / 2, -hi / 3])[np.arange(rows) % 6]
    return g, o


def shapes():
    """(name, matrix, mix_offset or None, interleave): every shape of the file's small-shape test"""
    rng = np.random.default_rng(11)
    blocks, iq_off = mref.iq_blocks(3, 12)
    hole = mref.band(3 * T, 1, 13)
    hole[T:2 * T] = 0.0
    hole_off = rng.uniform(-1, 1, 3 * T)
    hole_off[T + 1], hole_off[T + 2] = 7.5, -7.5         # rows without terms are the code of their offset: these two clip
    out = [('1x1', np.array([[-1.75]]), [0.5], 1),
           ('permutation-5', mref.permutation(5, 14)[0], None, 1),
           ('iq-6-k1', mref.block_diagonal(blocks), iq_off, 1),
           ('iq-6-k2', mref.block_diagonal(blocks), iq_off, 2)]
    out += [(f'tridiagonal-{r}-k1', mref.band(r, 1, 15 + r), rng.uniform(-1, 1, r), 1) for r in (T - 1, T, T + 1, 2 * T + 1)]
    out += [(f'tridiagonal-{r}-k2', mref.band(r, 1, 25 + r), rng.uniform(-1, 1, r), 2) for r in (T - 2, T, T + 2, 2 * T + 2)]
    out += [('dense-19x17-k1', mref.dense(19, 17, 16) / 4, rng.uniform(-1, 1, 19), 1),
            ('dense-18x17-k2', mref.dense(18, 17, 16) / 4, rng.uniform(-1, 1, 18), 2)]
    out += [(f'long-row-{k}', mref.one_long_row(T + 3, k, 5, 17 + k), None, 1) for k in (9, 17, 40)]
    out += [('empty-tile-k1', hole, hole_off, 1), ('empty-tile-k2', hole, hole_off, 2),
            ('3x11', mref.dense(3, 11, 18) * (rng.uniform(size=(3, 11)) < 0.6), [0.0, -0.0, 1.0], 1),
            ('11x3', mref.dense(11, 3, 19) * (rng.uniform(size=(11, 3)) < 0.6), None, 1),
            ('4x11-k2', mref.dense(4, 11, 20) * (rng.uniform(size=(4, 11)) < 0.6), None, 2)]
    return out


SHAPES = shapes()
BY_NAME = {s[0]: s for s in SHAPES}


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}')


def fused(x, m, mo, g, o, bits=16, shift=0, k=1, counts=True):
    """x (rows_in, n) NumPy -> (codes, counts or None) of a fused stage built for it, counts from a tensor of garbage"""
    st = distortion.MixDacStage(m, x.shape[1], g, mix_offset=mo, dac_offset=o, bits=bits, shift=shift, interleave=k,
                                dtype=x.dtype)
    try:
        c = torch.full((st.rows_out, 3), 0x5a5a5a5a5a, dtype=torch.int64, device=dev()) if counts else None
        y = st.apply_torch(torch.from_numpy(x).to(dev()), counts=c)
        assert y.dtype == torch.int16 and tuple(y.shape) == (st.out_rows, st.out_n) and y.is_contiguous()
        return y.cpu().numpy(), (c.cpu().numpy() if counts else None)
    finally:
        st.close()


def two_stages(x, m, mo, g, o, bits=16, shift=0, k=1):
    """the same through MixStage and DacStage, two launches on the device -> (codes, counts)"""
    mix = distortion.MixStage(m, x.shape[1], offset=mo, dtype=x.dtype)
    dac = distortion.DacStage(g, x.shape[1], offset=o, bits=bits, shift=shift, interleave=k, dtype=x.dtype,
                              batch=mix.rows_out)
    try:
        c = torch.full((mix.rows_out, 3), -1, dtype=torch.int64, device=dev())
        y = dac.apply_torch(mix.apply_torch(torch.from_numpy(x).to(dev())), counts=c)
        return y.cpu().numpy(), c.cpu().numpy()
    finally:
        mix.close()
        dac.close()


def check(x, m, mo, g, o, bits=16, shift=0, k=1, what=''):
    """fused == referee == two launches, codes and counts -> (codes, counts)"""
    codes, counts = fused(x, m, mo, g, o, bits, shift, k)
    want, want_counts = ref.mix_dac_ref(x, m, mo, g, o, bits, shift, k)
    same(codes, want, f'codes against the referee {what}')
    same(counts, want_counts, f'counts against the referee {what}')
    dev_codes, dev_counts = two_stages(x, m, mo, g, o, bits, shift, k)
    same(codes, dev_codes, f'codes against MixStage + DacStage {what}')
    same(counts, dev_counts, f'counts against MixStage + DacStage {what}')
    return codes, counts


def test_the_shapes_are_what_they_are_named():
    for name, rows in (('dense-19x17-k1', 19), ('dense-18x17-k2', 18)):      # a partial tile, several chunks
        assert rows % T != 0 and mref.reads_of(BY_NAME[name][1], T) == -(-rows // T) * 17 and 17 > 2 * 8
    for k in (9, 17, 40):
        m = BY_NAME[f'long-row-{k}'][1]
        assert np.count_nonzero(m[5]) == k and sorted(np.count_nonzero(m, axis=1))[:-1] == [1] * (T + 2)
    hole = BY_NAME['empty-tile-k1'][1]
    assert not hole[T:2 * T].any() and hole[:T].any() and hole[2 * T:].any()
    for name, m, mo, k in SHAPES:
        assert m.shape[0] % k == 0, name
    assert SPAN * 1 == distortion.MixDacStage(np.eye(2), 8, 1.0).span
    assert SPAN * 2 == distortion.MixDacStage(np.eye(2), 8, 1.0, interleave=2).span


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', SIZES)
def test_small_shapes(n, kind):
    """every shape at one size and dtype, the three formats taken in turn; rows clip and NaN is counted where the
    referee counts it"""
    clipped = np.zeros(3, dtype=np.int64)
    for i, (name, m, mo, k) in enumerate(SHAPES):
        bits, shift = FORMATS[(i + n) % 3]
        x = mref.rows_input(m.shape[1], n, 100 + n, NP_OF[kind])
        g, o = gains_offsets(m.shape[0], bits)
        _, counts = check(x, m, mo, g, o, bits, shift, k, f'{name} n={n} {kind} bits={bits}')
        clipped += counts.sum(axis=0)
    assert clipped[0] > 0 and clipped[1] > 0, clipped     # the gains make rows clip on both rails
    if n >= 15:
        assert clipped[2] > 0, clipped


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_special_values_and_rows_without_terms(kind):
    """a NaN-filled input row is counted on exactly the rows that have a term on it and stays out of the others; the
    rows of a tile without terms are the code of their mix offset, and that constant clips on two of them"""
    n = 1025
    x = mref.rows_input(2 * T + 2, n, 7, NP_OF[kind], specials=False)
    x[T - 1] = np.nan                                    # the band couples it to rows T - 2, T - 1, T: two tiles
    m = mref.band(2 * T + 2, 1, 8)
    g, o = gains_offsets(2 * T + 2, 16)
    for k in (1, 2):
        codes, counts = check(x, m, None, g, o, k=k, what=f'NaN row {kind} k={k}')
        assert counts[:, 2].tolist() == [n if T - 2 <= r <= T else 0 for r in range(2 * T + 2)]
    name, hole, hole_off, _ = BY_NAME['empty-tile-k1']
    xh = mref.rows_input(3 * T, n, 9, NP_OF[kind])
    g, o = np.full(3 * T, 5000.0), np.full(3 * T, 0.25)
    codes, counts = check(xh, hole, hole_off, g, o, what=f'empty tile {kind}')
    want_rows = dac_rows_ref.dac_ref(np.asarray(hole_off, dtype=NP_OF[kind])[T:2 * T, None], 5000.0, 0.25)[0]
    assert np.all(codes[T:2 * T] == want_rows) and len(np.unique(want_rows)) == T
    assert counts[T + 1].tolist() == [0, n, 0] and counts[T + 2].tolist() == [n, 0, 0] and not counts[T + 3].any()


def test_order_and_contraction_in_the_mix_half():
    """rows on which a mixed value one ulp off gives another code (tests/test_mix_dac_cpu.py holds the builder to that):
    the mix half sums in ascending column with rounded products, alone and as row 5 of a tile whose input list has 11
    entries, two chunks, with the row's terms in both"""
    x, m = ref.tie_case(256)
    codes, counts = check(x, m, None, [ref.TIE_GAIN], [ref.TIE_OFFSET], what='tie case')
    assert not counts.any() and len(np.unique(codes)) >= 200
    other_order = ref.mix_dac_ref(x[::-1], m[:, ::-1], None, ref.TIE_GAIN, ref.TIE_OFFSET)[0]
    assert np.all(other_order[0] != codes[0])
    contracted = np.array([ref.tie_code(mref.fused(x[:, i], m[0])) for i in range(x.shape[1])])
    assert np.all(contracted != codes[0])
    wide, t = np.zeros((T, 11)), T - 1                    # the last row of a tile: the Q of its pair
    wide[t, [1, 4, 9]] = m[0]                             # its terms in two chunks, other rows' terms between them
    for i, c in enumerate((0, 2, 3, 5, 6, 7, 8, 10)):
        wide[i % (T - 1), c] = (0.5, -0.25, 2.0)[i % 3]
    assert mref.reads_of(wide, T) == 11 and np.count_nonzero(wide[t]) == 3
    xw = mref.rows_input(11, 256, 21, specials=False)
    xw[[1, 4, 9]] = x
    g, o = np.full(T, 1000.0), np.zeros(T)
    g[t], o[t] = ref.TIE_GAIN, ref.TIE_OFFSET
    for k in (1, 2):
        inside, _ = check(xw, wide, None, g, o, k=k, what=f'tie case inside a tile k={k}')
        row = inside[t] if k == 1 else inside[t // 2, 1::2]
        assert np.array_equal(row, codes[0])


def test_contraction_and_rounding_mode_in_the_dac_half():
    """dac_rows_ref's exact ties after two roundings through an identity mix: a contracted multiply-add or
    round-half-away in the DAC half gives other codes; float32 ties for the rounding mode"""
    gq, M = 9731.37, 20000
    x, ks = dac_rows_ref.sensitive_row(1024, gq, M, seed=7)
    xx = np.stack([x, x[::-1].copy()])
    for k in (1, 2):
        codes, counts = check(xx, np.eye(2), None, [gq, gq], [-float(M)] * 2, k=k, what=f'sensitive rows k={k}')
        assert not counts.any()
    assert np.array_equal(fused(x[None], np.eye(1), None, [gq], [-float(M)])[0][0], np.rint(ks + 0.5).astype(np.int16))
    x32, ks32, g32 = dac_rows_ref.tie_row32()
    for off in (0.0, 7.0, -20000.0):
        codes, counts = check(x32[None], np.eye(1), None, [g32], [off], what=f'float32 ties offset={off}')
        assert np.array_equal(codes[0], np.rint(ks32 + 0.5 + off).astype(np.int16)) and not counts.any()


def test_float32_plans_round_the_mixed_row_to_float32_once():
    """mixed values 768 + small in float32 (ulp 2**-14) under a gain of 2**15 and an offset of -768 * 2**15: rounded to
    float32 the mixed value gives even codes only, so a mixed row that is NOT rounded before the converter gives other
    codes on many samples (found with the referee)"""
    n = 4099
    x = (mref.rows_input(4, n, 41, np.float32, specials=False) * np.float32(0.2)).astype(np.float32)
    m = mref.dense(2, 4, 42)
    mo, g, o = [768.0, 768.0], [2.0**15] * 2, [-768.0 * 2.0**15] * 2
    for k in (1, 2):
        codes, counts = check(x, m, mo, g, o, k=k, what=f'float32 rounding k={k}')
        unrounded = dac_rows_ref.dac_ref(mref.mix_ref(x.astype(np.float64), m, mo), g, o, interleave=k)[0]
        differ = int(np.count_nonzero(unrounded != codes))
        assert differ > n // 10 and not counts.any(), differ
        assert len(np.unique(codes)) > 1000


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', [5, 1024, 4101])
def test_windows_and_guards(n, kind):
    """both sides as windows at an odd element offset of wider tensors with odd row strides (the rows of a tile
    alternate in alignment; a pair row starts at an odd code): the guards of both sides stay, compared as bits, and the
    input is bit for bit what was put there"""
    dtype = NP_OF[kind]
    for name in ('iq-6-k2', 'iq-6-k1', f'tridiagonal-{2 * T + 1}-k1', 'dense-18x17-k2', 'long-row-17'):
        _, m, mo, k = BY_NAME[name]
        x = mref.rows_input(m.shape[1], n, 300 + n, dtype)
        g, o = gains_offsets(m.shape[0], 14)
        want, want_counts = ref.mix_dac_ref(x, m, mo, g, o, 14, 2, k)
        src, dst = Window(m.shape[1], n, dtype, x), Window(m.shape[0] // k, k * n, np.int16)
        st = distortion.MixDacStage(m, n, g, mix_offset=mo, dac_offset=o, bits=14, shift=2, interleave=k, dtype=dtype)
        counts = torch.full((m.shape[0], 3), -77, dtype=torch.int64, device=dev())
        assert st.apply_torch(src.win, dst.win, counts).data_ptr() == dst.ptr
        torch.cuda.synchronize()
        same(dst.host(), want, f'window {name} n={n} {kind}')
        same(counts.cpu().numpy(), want_counts, f'window counts {name} n={n} {kind}')
        dst.assert_guards()
        src.assert_holds(x)
        st.close()


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_every_output_lead_into_a_sentinel_filled_tensor(kind, k):
    """code rows at every lead 0 .. 7 into a 16-byte group (odd ones under K = 2 too), input rows 8 and 40 bytes into a
    wider buffer: [0, k n) of every code row is written -- rows without terms too -- and the sentinels before, after
    and between the rows stay; a second apply overwrites the counts"""
    dtype = NP_OF[kind]
    name, m, mo, _ = BY_NAME[f'empty-tile-k{k}']
    rows = m.shape[0]
    g, o = gains_offsets(rows, 14)
    for n in (3, SPAN + 1):
        x = mref.rows_input(m.shape[1], n, 500 + n, dtype)
        want, want_counts = ref.mix_dac_ref(x, m, mo, g, o, 14, 2, k)
        assert not np.any(want == SENTINEL)
        st = distortion.MixDacStage(m, n, g, mix_offset=mo, dac_offset=o, bits=14, shift=2, interleave=k, dtype=dtype)
        for lead in range(8):
            off = (8 if lead % 2 == 0 else 40) // np.dtype(dtype).itemsize
            wide = torch.full((m.shape[1], n + 37), 7.0, dtype=TORCH_OF[kind], device=dev())
            win = wide[:, off:off + n]
            win.copy_(torch.from_numpy(x))
            out = torch.full((rows // k, k * n + 64), SENTINEL, dtype=torch.int16, device=dev())
            counts = torch.full((rows, 3), -77, dtype=torch.int64, device=dev())
            res = st.apply_torch(win, out[:, lead:lead + k * n], counts)
            assert res.data_ptr() == out[:, lead:].data_ptr() and tuple(res.shape) == (rows // k, k * n)
            full = out.cpu().numpy()
            same(full[:, lead:lead + k * n], want, f'{name} n={n} lead={lead} {kind}')
            assert np.all(full[:, :lead] == SENTINEL) and np.all(full[:, lead + k * n:] == SENTINEL)
            same(counts.cpu().numpy(), want_counts, f'counts {name} n={n} lead={lead} {kind}')
            st.apply_torch(win, out[:, lead:lead + k * n], counts)
            same(counts.cpu().numpy(), want_counts, f'counts of a second apply {name} n={n} lead={lead} {kind}')
        st.close()


@pytest.mark.parametrize('kind,side', [('f64', 'far_in'), ('f64', 'far_out')])
def test_rows_more_than_2_pow_32_elements_apart(kind, side):
    dtype, n = NP_OF[kind], 4099
    m, mo = np.array([[1.02, -0.07], [0.05, 0.97]]), [0.01, -0.02]
    g, o = [30000.0, -28000.0], [0.5, -3.25]
    x = mref.rows_input(2, n, 900, dtype)
    want, want_counts = ref.mix_dac_ref(x, m, mo, g, o)
    st = distortion.MixDacStage(m, n, g, mix_offset=mo, dac_offset=o, dtype=dtype)
    src = dst = None
    try:
        if side == 'far_in':
            src, dst = FarWindow(n, dtype, x), Window(2, n, np.int16)
        else:
            src, dst = Window(2, n, dtype, x), FarWindow(n, np.int16)
        assert max(src.stride, dst.stride) > 2**32
        counts = torch.full((2, 3), 5, dtype=torch.int64, device=dev())
        assert st.apply_torch(src.win, dst.win, counts).data_ptr() == dst.ptr
        torch.cuda.synchronize()
        same(dst.host(), want, f'far rows {kind} {side}')
        same(counts.cpu().numpy(), want_counts, f'far rows counts {kind} {side}')
        dst.assert_guards()
        src.assert_holds(x)
    finally:
        st.close()
        del src, dst
        free_far_arena()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_plain_build_against_counting_build(kind):
    n = SPAN + 5
    for name in ('iq-6-k2', f'tridiagonal-{2 * T + 1}-k1'):
        _, m, mo, k = BY_NAME[name]
        x = mref.rows_input(m.shape[1], n, 650, NP_OF[kind])
        g, o = gains_offsets(m.shape[0], 12)
        plain, none = fused(x, m, mo, g, o, 12, 4, k, counts=False)
        counted, counts = fused(x, m, mo, g, o, 12, 4, k)
        want, want_counts = ref.mix_dac_ref(x, m, mo, g, o, 12, 4, k)
        assert none is None
        same(plain, want, f'without counts {name} {kind}')
        same(counted, want, f'with counts {name} {kind}')
        same(counts, want_counts, f'counts {name} {kind}')
        assert want_counts.any()


def test_batch_independence():
    """a tile's rows give the same codes and counts alone and inside a larger matrix, whichever tile they land in"""
    n = 4099
    blocks, iq_off = mref.iq_blocks(T // 2, 50)
    m = mref.block_diagonal(blocks)
    x = mref.rows_input(T, n, 51)
    g, o = gains_offsets(T, 16)
    for k in (1, 2):
        alone, c_alone = check(x, m, iq_off, g, o, k=k, what=f'alone k={k}')
        other, other_off = mref.band(T + 2, 1, 52), np.linspace(-1, 1, T + 2)
        big = mref.block_diagonal([other, m, other])
        xo = mref.rows_input(T + 2, n, 53)
        go, oo = gains_offsets(T + 2, 16)
        codes, counts = check(np.vstack([xo, x, xo]), big, np.r_[other_off, iq_off, other_off], np.r_[go, g, go],
                              np.r_[oo, o, oo], k=k, what=f'inside k={k}')
        lo = (T + 2) // k
        assert np.array_equal(codes[lo:lo + T // k], alone) and np.array_equal(counts[T + 2:2 * T + 2], c_alone)


def test_side_stream_equals_default_stream():
    name, m, mo, k = BY_NAME['dense-18x17-k2']
    n = 4099
    x = mref.rows_input(m.shape[1], n, 600)
    g, o = gains_offsets(m.shape[0], 16)
    st = distortion.MixDacStage(m, n, g, mix_offset=mo, dac_offset=o, interleave=k)
    ca = torch.empty((m.shape[0], 3), dtype=torch.int64, device=dev())
    a = st.apply_torch(torch.from_numpy(x).to(dev()), counts=ca).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z = torch.from_numpy(x).to(dev())
        cb = torch.full((m.shape[0], 3), 99, dtype=torch.int64, device=dev())
        b = st.apply_torch(z, counts=cb) + 0                       # produced and consumed on the side stream
        cb = cb + 0
    side.synchronize()
    want, want_counts = ref.mix_dac_ref(x, m, mo, g, o, interleave=k)
    same(a, want, 'default stream')
    same(b.cpu().numpy(), want, 'side stream')
    same(ca.cpu().numpy(), want_counts, 'default stream, counts')
    same(cb.cpu().numpy(), want_counts, 'side stream, counts')
    st.close()


@pytest.mark.parametrize('kind,k', [('f64', 2), ('f32', 1)])
def test_graph_replay_equals_eager(kind, k):
    """one apply captured (no allocation, no synchronisation inside it: the capture would refuse) and replayed on fresh
    feeds: codes and counts are those of an eager apply of a twin stage on the same feed; the counts are overwritten by
    every replay, not added to"""
    n = SPAN + 3
    name, m, mo, _ = BY_NAME['iq-6-k2'] if k == 2 else BY_NAME[f'tridiagonal-{T + 1}-k1']
    g, o = gains_offsets(m.shape[0], 14)
    make = lambda: distortion.MixDacStage(m, n, g, mix_offset=mo, dac_offset=o, bits=14, shift=2, interleave=k,
                                          dtype=NP_OF[kind])
    st, twin = make(), make()
    x = torch.empty((m.shape[1], n), dtype=TORCH_OF[kind], device=dev())
    out = torch.empty((m.shape[0] // k, k * n), dtype=torch.int16, device=dev())
    counts = torch.empty((m.shape[0], 3), dtype=torch.int64, device=dev())
    feeds = [[mref.rows_input(m.shape[1], n, 700 + i, NP_OF[kind])] for i in range(2)]
    got = graph_replay.replay(lambda: st.apply_torch(x, out, counts), [x], feeds, [out, counts])
    for i, feed in enumerate(feeds):
        want, want_counts = ref.mix_dac_ref(feed[0], m, mo, g, o, 14, 2, k)
        eager = graph_replay.eager(lambda: twin.apply_torch(x, out, counts), [x], feed, [out, counts])
        same(got[i][0], want, f'replay {i} codes {kind} k={k}')
        same(got[i][1], want_counts, f'replay {i} counts {kind} k={k}')
        same(eager[0], got[i][0], f'eager codes {i}')
        same(eager[1], got[i][1], f'eager counts {i}')
        assert want_counts.any()
    st.close()
    twin.close()


def test_overlap_and_refused_tensors():
    n, rows = 256, 4
    m = mref.dense(rows, 5, 1)
    st = distortion.MixDacStage(m, n, 1000.0, interleave=2)
    buf = torch.zeros(5 * n + 64, dtype=torch.float64, device=dev())
    x = buf[:5 * n].view(5, n)
    as_codes = buf.view(torch.int16)                                      # the same bytes as int16
    out = torch.zeros((2, 2 * n), dtype=torch.int16, device=dev())
    counts = torch.zeros((rows, 3), dtype=torch.int64, device=dev())
    st.apply_torch(x, out, counts)                                        # fine
    for bad_out in (as_codes[:2 * 2 * n].view(2, 2 * n), as_codes[4 * 5 * n - 2 * 2 * n + 8:][:2 * 2 * n].view(2, 2 * n)):
        with pytest.raises(ValueError, match='mix dac stage is out of place: out overlaps x'):
            st.apply_torch(x, bad_out, counts)
    over_x = buf[8:8 + rows * 3].view(torch.int64).view(rows, 3)
    over_out = out.view(-1)[16:16 + rows * 12].view(torch.int64).view(rows, 3)
    for bad_counts in (over_x, over_out):
        with pytest.raises(ValueError, match='mix dac stage: counts overlaps x / out'):
            st.apply_torch(x, out, bad_counts)
    wide = torch.zeros((rows, 4), dtype=torch.int64, device=dev())
    for bad_counts in (counts[:3], counts.view(-1), wide[:, :3], counts.to(torch.int32), counts.cpu(),
                       torch.zeros((rows, 2), dtype=torch.int64, device=dev())):
        with pytest.raises(ValueError, match='counts'):
            st.apply_torch(x, out, bad_counts)
    xc = torch.zeros((5, n), dtype=torch.float64, device=dev())
    for bad in (xc[:4], xc[:, :n - 1], xc.to(torch.float32), xc.cpu(), xc.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected x'):
            st.apply_torch(bad, out)
    for bad in (out[:1], out[:, :2 * n - 1], out.to(torch.int32), out.cpu(), out.t().contiguous().t(),
                torch.zeros((rows, n), dtype=torch.int16, device=dev())):
        with pytest.raises(ValueError, match='expected out'):
            st.apply_torch(xc, bad)
    # the C side's own checks through the raw pointers: WFK_EINVAL, the stage named, nothing launched
    lib, h = _engine.lib(), st.plan._h
    out.fill_(SENTINEL)
    counts.fill_(7)
    X, Y, Cn = xc.data_ptr(), out.data_ptr(), counts.data_ptr()
    for args, message in (((None, n, Y, 2 * n, None), b'null in / out'),
                          ((X, n, None, 2 * n, None), b'null in / out'),
                          ((X + 4, n, Y, 2 * n, None), b'not aligned to their element'),
                          ((X, n, Y + 1, 2 * n, None), b'not aligned to their element'),
                          ((X, n - 1, Y, 2 * n, None), b'in row stride smaller'),
                          ((X, n, Y, 2 * n - 1, None), b'out row stride smaller'),
                          ((X, n, X + 8, 2 * n, None), b'mix dac is out of place: out overlaps in'),
                          ((X, n, Y, 2 * n, Cn + 4), b'counts are not aligned'),
                          ((X, n, Y, 2 * n, X + 16), b'counts overlaps in'),
                          ((X, n, Y, 2 * n, Y + 8), b'counts overlaps out')):
        assert lib.wfk_mix_dac_apply(h, *args, None) == -1, args
        text = lib.wfk_last_error()
        assert text.startswith(b'mix dac') and message in text, (args, text)
        with pytest.raises(_engine.EngineError, match=message.decode()):
            st.apply(*args)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL) and np.all(counts.cpu().numpy() == 7)
    st.close()
    empty = distortion.MixDacStage(np.eye(2), 0, [1.0, 2.0], interleave=2)   # n = 0: no kernel; the counts are zeroed
    e = torch.zeros((2, 0), dtype=torch.float64, device=dev())
    c = torch.full((2, 3), 5, dtype=torch.int64, device=dev())
    assert tuple(empty.apply_torch(e, counts=c).shape) == (1, 0)
    assert not c.cpu().numpy().any()
    assert lib.wfk_mix_dac_apply(empty.plan._h, None, 0, None, 0, None, None) == 0
    empty.close()


def test_consistency_of_the_entry_points():
    n = 3001
    for name, m, mo, k in SHAPES:
        for kind in ('f64', 'f32'):
            st = distortion.MixDacStage(m, n, 1000.0, mix_offset=mo, interleave=k, bits=14, shift=1, dtype=NP_OF[kind])
            assert st.kernel_name() == st.kernel_name(counts=False) == f'mix_dac_rows<{NAME_OF[kind]},{k},false>'
            assert st.kernel_name(counts=True) == f'mix_dac_rows<{NAME_OF[kind]},{k},true>'
            assert st.reads == st.plan.library_reads() == mref.reads_of(m, T), name
            assert (st.rows_out, st.rows_in, st.nnz, st.n) == (m.shape[0], m.shape[1], np.count_nonzero(m), n)
            assert (st.out_rows, st.out_n, st.lo, st.hi, st.span) == (m.shape[0] // k, k * n, -8192, 8191, SPAN * k)
            assert st.gain.tolist() == [1000.0] * m.shape[0] and st.offset.tolist() == [0.0] * m.shape[0]
            st.close()
    blocks, mo = mref.iq_blocks(5, 30)
    dense = mref.block_diagonal(blocks)
    x = mref.rows_input(10, n, 31)
    g, o = gains_offsets(10, 16)
    want, want_counts = ref.mix_dac_ref(x, dense, mo, g, o, interleave=2)
    a = distortion.MixDacStage.from_blocks(blocks, n, g, mix_offset=mo, dac_offset=o, interleave=2)
    assert (a.reads, a.nnz, a.rows_out, a.rows_in, a.out_rows) == (10, 20, 10, 10, 5)
    same(a.apply_torch(torch.from_numpy(x).to(dev())).cpu().numpy(), want, 'from_blocks')
    a.close()
    fs = np.linspace(0.7, 1.3, 10)
    b = distortion.MixDacStage.from_full_scale(dense, n, fs, mix_offset=mo, bits=14, shift=2)
    assert np.array_equal(b.gain, 8191 / fs)
    same(b.apply_torch(torch.from_numpy(x).to(dev())).cpu().numpy(),
         ref.mix_dac_ref(x, dense, mo, 8191 / fs, 0.0, 14, 2)[0], 'from_full_scale')
    b.close()
    for sig in (x, x.astype(np.float32)):
        codes, counts = distortion.mix_dac_rows(sig, dense, g, mo, o, interleave=2, return_counts=True)
        w, wc = ref.mix_dac_ref(sig, dense, mo, g, o, interleave=2)
        same(codes, w, f'mix_dac_rows {sig.dtype}')
        same(counts, wc, f'mix_dac_rows counts {sig.dtype}')
        same(distortion.mix_dac_rows(sig, dense, 20000.0, bits=16), ref.mix_dac_ref(sig, dense, None, 20000.0)[0],
             f'mix_dac_rows, one gain {sig.dtype}')
    if importlib.util.find_spec('scipy') is not None:
        import scipy.sparse as sp
        tri = mref.band(2 * T + 1, 1, 33)
        c = distortion.MixDacStage(sp.csr_matrix(tri), n, 25000.0)
        assert (c.nnz, c.reads) == (np.count_nonzero(tri), mref.reads_of(tri, T))
        xt = mref.rows_input(2 * T + 1, n, 34)
        same(c.apply_torch(torch.from_numpy(xt).to(dev())).cpu().numpy(), ref.mix_dac_ref(xt, tri, None, 25000.0)[0],
             'scipy.sparse matrix')
        c.close()


def test_plain_c_consumer_mixes_to_codes_on_the_device(tmp_path):
    exe = tmp_path / 'mix_dac_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'mix_dac_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'mixed to codes on the device, 16 codes ok' in r.stdout, r.stdout
