"""The per-row IIR stage that ends in DAC codes on the device (distortion.IirDacStage / iir_dac_rows,
csrc/wfk_iir_rows_dac.hip) against the two stages it replaces, IirStage followed by DacStage on the same device -- codes,
counts and zf bit for bit, no tolerance -- and against the NumPy referee (tests/iir_dac_ref.py), where a code may differ
by one step at an UNDECIDED sample and nowhere else (the rule is spelt in the referee's module; that the share of such
samples is small is held, from the referee alone, by tests/test_iir_dac_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from cases import FP64_IIR_TOL
import graph_replay
import iir_dac_ref as ref
from row_windows import FarWindow, Window, free_far_arena
from waveforms_amd import _engine, _rows, distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_OF = {'f64': np.float64, 'f32': np.float32}
TORCH_OF = {'f64': torch.float64, 'f32': torch.float32}
TILE = ref.TILE
SENTINEL = -21846                                        # 0xAAAA
KERNELS = [f'iir_rows_dac<{t},{s},{o}>' for t in ('f64', 'f32') for s, o in ref.SHAPES]


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}')


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def two_launches(rows, x, gain, offset, bits=16, shift=0, initial=0.0, zi=None):
    """IirStage, then DacStage, on the device -> (codes, counts, zf) host arrays"""
    batch, n = x.shape
    iir = distortion.IirStage(rows, n, batch, dtype=x.dtype)
    dac = distortion.DacStage(gain, n, offset=offset, bits=bits, shift=shift, dtype=x.dtype, batch=batch)
    try:
        zf = torch.full((batch, iir.state_dim), 9.0, dtype=torch.float64, device=dev())
        c = torch.full((batch, 3), -1, dtype=torch.int64, device=dev())
        z = iir.apply_torch(to_dev(x), out=torch.empty((batch, n), dtype=_rows.torch_dtype(x.dtype), device=dev()),
                            initial=initial, zi=None if zi is None else to_dev(zi), zf=zf)
        y = dac.apply_torch(z, counts=c)
        return y.cpu().numpy(), c.cpu().numpy(), zf.cpu().numpy()
    finally:
        iir.close()
        dac.close()


def fused(rows, x, gain, offset, bits=16, shift=0, initial=0.0, zi=None, counts=True, stage=None):
    """the same through one IirDacStage, counts from a tensor of garbage -> (codes, counts or None, zf)"""
    batch, n = x.shape
    st = stage or distortion.IirDacStage(rows, n, gain, offset=offset, bits=bits, shift=shift, dtype=x.dtype)
    try:
        zf = torch.full((batch, st.state_dim), 9.0, dtype=torch.float64, device=dev())
        c = torch.full((batch, 3), 0x5a5a5a5a5a, dtype=torch.int64, device=dev()) if counts else None
        y = st.apply_torch(to_dev(x), counts=c, initial=initial, zi=None if zi is None else to_dev(zi), zf=zf)
        assert y.dtype == torch.int16 and tuple(y.shape) == (batch, n)
        return y.cpu().numpy(), (c.cpu().numpy() if counts else None), zf.cpu().numpy()
    finally:
        if stage is None:
            st.close()


# ---- against the two launches: exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('nsec,order', ref.SHAPES)
def test_codes_counts_and_zf_equal_the_two_launches(nsec, order, kind):
    """every length, batch and format of the referee's lists: gains of both signs that clip rows on both rails,
    fractional offsets, per-row levels, a zi"""
    clipped = np.zeros(2, dtype=np.int64)
    for n in ref.LENGTHS:
        for batch in ref.BATCHES:
            for bits, shift in ref.FORMATS:
                case = ref.Case(nsec, order, batch, n, bits, shift, dtype=NP_OF[kind])
                what = f'({nsec},{order}) {kind} n={n} batch={batch} bits={bits} shift={shift}'
                a = fused(case.rows, case.x, case.gain, case.offset, bits, shift, case.initial, case.zi)
                b = two_launches(case.rows, case.x, case.gain, case.offset, bits, shift, case.initial, case.zi)
                same(a[0], b[0], f'codes {what}')
                same(a[1], b[1], f'counts {what}')
                same(a[2], b[2], f'zf {what}')
                if n >= TILE:
                    assert (a[1][:, 0] > 0).all() and (a[1][:, 1] > 0).all(), what     # both rails, every row
                clipped += a[1][:, :2].sum(axis=0)
    assert clipped.all()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_kernel_names_and_consistency_of_the_entry_points(kind):
    n = 3001
    for nsec, order in ref.SHAPES:
        case = ref.Case(nsec, order, 2, 16, dtype=NP_OF[kind])
        st = distortion.IirDacStage(case.rows, 16, 100.0, bits=14, shift=1, dtype=NP_OF[kind])
        assert st.kernel_name() == f'iir_rows_dac<{kind},{nsec},{order}>' and st.kernel_name() in KERNELS
        assert (st.n, st.batch, st.state_dim, st.lo, st.hi, st.bits, st.shift) == (16, 2, nsec * order, -8192, 8191, 14, 1)
        assert st.gain.tolist() == [100.0, 100.0] and st.offset.tolist() == [0.0, 0.0]
        st.close()
    case = ref.Case(1, 3, 3, n, dtype=NP_OF[kind])
    want = two_launches(case.rows, case.x, case.gain, case.offset, initial=case.initial)
    codes, counts = distortion.iir_dac_rows(case.x, case.rows, case.gain, case.offset, initial=case.initial,
                                            return_counts=True)
    same(codes, want[0], 'iir_dac_rows')
    same(counts, want[1], 'iir_dac_rows counts')
    same(distortion.iir_dac_rows(case.x, case.rows, 2000.0), two_launches(case.rows, case.x, 2000.0, 0.0)[0],
         'iir_dac_rows, one gain')
    # from_full_scale; ONE cascade for every row, as a list and as an SOS matrix
    fs = np.array([0.7, 1.0, 1.3])
    st = distortion.IirDacStage.from_full_scale(case.rows, n, fs, bits=14, shift=2, dtype=NP_OF[kind])
    assert np.array_equal(st.gain, 8191 / fs)
    same(fused(None, case.x, None, None, stage=st)[0], two_launches(case.rows, case.x, 8191 / fs, 0.0, 14, 2)[0],
         'from_full_scale')
    st.close()
    one = case.rows[0]
    st = distortion.IirDacStage(one, n, [900.0, -800.0, 700.0], dtype=NP_OF[kind])
    assert st.batch == 3
    same(fused(None, case.x, None, None, stage=st)[0], two_launches([one] * 3, case.x, [900.0, -800.0, 700.0], 0.0)[0],
         'one cascade for every row')
    st.close()
    sos = np.array([[0.2, 0.1, 0.05, 1.0, -1.2, 0.4], [1.0, -0.4, 0.1, 1.0, -0.9, 0.3]])
    st = distortion.IirDacStage(sos, n, 3000.0, batch=3, dtype=NP_OF[kind])
    assert st.kernel_name() == f'iir_rows_dac<{kind},2,2>'
    same(fused(None, case.x, None, None, stage=st)[0],
         two_launches([_engine.sos_sections(sos)] * 3, case.x, 3000.0, 0.0)[0], 'an SOS matrix for every row')
    st.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('what', ['nan', 'inf'])
def test_a_non_finite_sample_in_mid_row(what, kind):
    """the state is NaN from there on (an Inf: from the first Inf - Inf of the recurrence on): the codes behind it are
    0 and are counted as NaN, as the two launches give them"""
    n, at = 2 * TILE + 77, TILE + 1234
    case = ref.Case(1, 2, 3, n, dtype=NP_OF[kind])
    x = case.x.copy()
    x[1, at] = np.nan if what == 'nan' else np.inf
    a = fused(case.rows, x, case.gain, case.offset, initial=case.initial)
    b = two_launches(case.rows, x, case.gain, case.offset, initial=case.initial)
    same(a[0], b[0], f'codes {what}')
    same(a[1], b[1], f'counts {what}')
    same(a[2], b[2], f'zf {what}')
    clean = fused(case.rows, case.x, case.gain, case.offset, initial=case.initial)
    same(a[0][[0, 2]], clean[0][[0, 2]], 'the other rows')
    same(a[0][1, :at], clean[0][1, :at], 'the row in front of the sample')
    tail = 16 if what == 'inf' else 0                   # an Inf is a NaN in every lane run behind its own (16 samples)
    assert not a[0][1, at + tail:].any()
    assert n - at - tail <= a[1][1, 2] <= n - at and not a[1][[0, 2], 2].any()


# ---- against the referee ------------------------------------------------------------------------------------------------
def test_codes_differ_from_the_referee_only_at_undecided_samples():
    for case in ref.referee_cases():
        what = f'({case.nsec},{case.order}) n={case.n} bits={case.bits}'
        codes, counts, zf = fused(case.rows, case.x, case.gain, case.offset, case.bits, case.shift, case.initial, case.zi)
        want, want_counts = case.reference()
        mask, near_lo, near_hi = case.undecided()
        diff = codes.astype(np.int64) - want.astype(np.int64)
        print(f'{what}: {np.count_nonzero(diff)} codes differ, {int(mask.sum())} undecided')
        assert not diff[~mask].any(), (what, np.argwhere((diff != 0) & ~mask)[:4])
        assert np.all(np.abs(diff) <= 1 << case.shift), what
        cd = np.abs(counts - want_counts)
        assert (cd[:, 0] <= near_lo.sum(axis=1)).all() and (cd[:, 1] <= near_hi.sum(axis=1)).all(), (what, cd)
        assert not counts[:, 2].any()
        scale = np.maximum(1.0, np.abs(case.zf).max(axis=1))
        assert (np.abs(zf - case.zf).max(axis=1) <= 1e-9 * scale).all(), what


# ---- memory and reproducibility ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', [5, 1024, TILE + 5])
def test_windows_and_guards(n, kind):
    """both sides as windows at an odd element offset of wider tensors with odd row strides: consecutive code rows
    alternate between aligned and unaligned slots.  The guards of both sides stay, compared as bits, and the input is
    bit for bit what was put there"""
    dtype = NP_OF[kind]
    case = ref.Case(1, 3, 5, n, 14, 2, dtype=dtype)
    want = two_launches(case.rows, case.x, case.gain, case.offset, 14, 2, case.initial)
    src, dst = Window(5, n, dtype, case.x), Window(5, n, np.int16)
    st = distortion.IirDacStage(case.rows, n, case.gain, offset=case.offset, bits=14, shift=2, dtype=dtype)
    counts = torch.full((5, 3), -77, dtype=torch.int64, device=dev())
    assert st.apply_torch(src.win, dst.win, counts, initial=case.initial).data_ptr() == dst.ptr
    torch.cuda.synchronize()
    same(dst.host(), want[0], f'window n={n} {kind}')
    same(counts.cpu().numpy(), want[1], f'window counts n={n} {kind}')
    dst.assert_guards()
    src.assert_holds(case.x)
    st.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_every_lead_of_a_code_row_into_a_sentinel_filled_tensor(kind):
    """code rows at every lead 0 .. 7 into a 16-byte group: [0, n) of every row is written, the sentinels before, after
    and between the rows stay; a second apply overwrites the counts"""
    dtype = NP_OF[kind]
    for n in (3, 2 * TILE + 9):
        case = ref.Case(2, 1, 3, n, dtype=dtype)
        want = two_launches(case.rows, case.x, case.gain, case.offset, initial=case.initial)
        assert not np.any(want[0] == SENTINEL)
        st = distortion.IirDacStage(case.rows, n, case.gain, offset=case.offset, dtype=dtype)
        x = to_dev(case.x)
        for lead in range(8):
            out = torch.full((3, n + 64), SENTINEL, dtype=torch.int16, device=dev())
            counts = torch.full((3, 3), -77, dtype=torch.int64, device=dev())
            res = st.apply_torch(x, out[:, lead:lead + n], counts, initial=case.initial)
            assert res.data_ptr() == out[:, lead:].data_ptr() and tuple(res.shape) == (3, n)
            full = out.cpu().numpy()
            same(full[:, lead:lead + n], want[0], f'n={n} lead={lead} {kind}')
            assert np.all(full[:, :lead] == SENTINEL) and np.all(full[:, lead + n:] == SENTINEL)
            same(counts.cpu().numpy(), want[1], f'counts n={n} lead={lead} {kind}')
            st.apply_torch(x, out[:, lead:lead + n], counts, initial=case.initial)
            same(counts.cpu().numpy(), want[1], f'counts of a second apply n={n} lead={lead} {kind}')
        st.close()


@pytest.mark.parametrize('kind,side', [('f64', 'far_in'), ('f64', 'far_out'), ('f32', 'far_out')])
def test_rows_more_than_2_pow_32_elements_apart(kind, side):
    dtype, n = NP_OF[kind], TILE + 3
    case = ref.Case(1, 3, 2, n, dtype=dtype)
    want = two_launches(case.rows, case.x, case.gain, case.offset, initial=case.initial)
    st = distortion.IirDacStage(case.rows, n, case.gain, offset=case.offset, dtype=dtype)
    src = dst = None
    try:
        if side == 'far_in':
            src, dst = FarWindow(n, dtype, case.x), Window(2, n, np.int16)
        else:
            src, dst = Window(2, n, dtype, case.x), FarWindow(n, np.int16)
        assert max(src.stride, dst.stride) > 2**32
        counts = torch.full((2, 3), 5, dtype=torch.int64, device=dev())
        assert st.apply_torch(src.win, dst.win, counts, initial=case.initial).data_ptr() == dst.ptr
        torch.cuda.synchronize()
        same(dst.host(), want[0], f'far rows {kind} {side}')
        same(counts.cpu().numpy(), want[1], f'far rows counts {kind} {side}')
        dst.assert_guards()
        src.assert_holds(case.x)
    finally:
        st.close()
        del src, dst
        free_far_arena()


def test_overlap_and_refused_tensors():
    n, rows = 256, 3
    case = ref.Case(1, 1, rows, n)
    st = distortion.IirDacStage(case.rows, n, 1000.0)
    buf = torch.zeros(rows * n + 64, dtype=torch.float64, device=dev())
    x = buf[:rows * n].view(rows, n)
    as_codes = buf.view(torch.int16)                                      # the same bytes as int16
    out = torch.zeros((rows, n), dtype=torch.int16, device=dev())
    counts = torch.zeros((rows, 3), dtype=torch.int64, device=dev())
    st.apply_torch(x, out, counts)                                        # fine
    for bad_out in (as_codes[:rows * n].view(rows, n), as_codes[4 * rows * n - rows * n + 8:][:rows * n].view(rows, n)):
        with pytest.raises(ValueError, match='iir dac stage is out of place: codes overlaps x'):
            st.apply_torch(x, bad_out, counts)
    over_x = buf[8:8 + rows * 3].view(torch.int64).view(rows, 3)
    over_out = out.view(-1)[16:16 + rows * 12].view(torch.int64).view(rows, 3)
    for bad_counts in (over_x, over_out):
        with pytest.raises(ValueError, match='iir dac stage: counts overlaps x / codes'):
            st.apply_torch(x, out, bad_counts)
    for bad_counts in (counts[:2], counts.view(-1), counts.to(torch.int32), counts.cpu()):
        with pytest.raises(ValueError, match='counts'):
            st.apply_torch(x, out, bad_counts)
    xc = torch.zeros((rows, n), dtype=torch.float64, device=dev())
    for bad in (xc[:2], xc[:, :n - 1], xc.to(torch.float32), xc.cpu(), xc.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected x'):
            st.apply_torch(bad, out)
    for bad in (out[:1], out[:, :n - 1], out.to(torch.int32), out.cpu(), out.t().contiguous().t()):
        with pytest.raises(ValueError, match='expected codes'):
            st.apply_torch(xc, bad)
    with pytest.raises(ValueError, match='zi / zf'):
        st.apply_torch(xc, out, zf=torch.zeros((rows, 2), dtype=torch.float64, device=dev()))
    # the C side's own checks through the raw pointers: WFK_EINVAL, the stage named, nothing launched
    lib, h = _engine.lib(), st.plan._h
    out.fill_(SENTINEL)
    counts.fill_(7)
    X, Y, Cn = xc.data_ptr(), out.data_ptr(), counts.data_ptr()
    for args, message in (((None, n, Y, n, None), b'null in / out'),
                          ((X, n, None, n, None), b'null in / out'),
                          ((X + 4, n, Y, n, None), b'not aligned to their element'),
                          ((X, n, Y + 1, n, None), b'not aligned to their element'),
                          ((X, n - 1, Y, n, None), b'in row stride smaller'),
                          ((X, n, Y, n - 1, None), b'out row stride smaller'),
                          ((X, n, X + 8, n, None), b'per-row IIR dac is out of place: out overlaps in'),
                          ((X, n, Y, n, Cn + 4), b'counts are not aligned'),
                          ((X, n, Y, n, X + 16), b'counts overlaps in'),
                          ((X, n, Y, n, Y + 8), b'counts overlaps out')):
        assert lib.wfk_iir_rows_dac_apply(h, *args, None, None, None, None) == -1, args
        text = lib.wfk_last_error()
        assert text.startswith(b'per-row IIR dac') and message in text, (args, text)
        with pytest.raises(_engine.EngineError, match=message.decode()):
            st.plan.apply(*args)
    assert lib.wfk_iir_rows_dac_apply_shared_in(h, X, X + 8, n, None, None, None, None, None) == -1
    assert b'shared input is out of place: out overlaps in' in lib.wfk_last_error()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL) and np.all(counts.cpu().numpy() == 7)
    st.close()
    empty = distortion.IirDacStage(case.rows, 0, 1.0)                     # n = 0: no kernel; the counts are zeroed
    e = torch.zeros((rows, 0), dtype=torch.float64, device=dev())
    c = torch.full((rows, 3), 5, dtype=torch.int64, device=dev())
    assert tuple(empty.apply_torch(e, counts=c).shape) == (rows, 0)
    assert not c.cpu().numpy().any()
    empty.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_permutation_repeatability_and_the_build_without_counts(kind):
    n = 2 * TILE + 100
    case = ref.Case(1, 3, 7, n, dtype=NP_OF[kind])
    perm = np.random.default_rng(1).permutation(7)
    a = fused(case.rows, case.x, case.gain, case.offset, initial=case.initial, zi=case.zi)
    b = fused(case.rows, case.x, case.gain, case.offset, initial=case.initial, zi=case.zi)
    p = fused([case.rows[i] for i in perm], case.x[perm], case.gain[perm], case.offset[perm], initial=case.initial[perm],
              zi=case.zi[perm])
    plain = fused(case.rows, case.x, case.gain, case.offset, initial=case.initial, zi=case.zi, counts=False)
    for i, name in enumerate(('codes', 'counts', 'zf')):
        same(a[i], b[i], f'two runs, {name}')
        same(p[i], a[i][perm], f'permuted rows, {name}')
    assert plain[1] is None
    same(plain[0], a[0], 'without counts')
    same(plain[2], a[2], 'zf without counts')
    assert a[1][:, :2].all()
    # a row alone gives what it gives inside the batch
    alone = fused(case.rows[3:4], case.x[3:4], case.gain[3:4], case.offset[3:4], initial=case.initial[3:4], zi=case.zi[3:4])
    same(alone[0], a[0][3:4], 'a row alone')
    same(alone[1], a[1][3:4], 'a row alone, counts')


@pytest.mark.parametrize('cut', [TILE + 1234, 2 * TILE])              # inside a tile / on a tile edge
def test_a_row_cut_in_two_gives_the_codes_of_the_whole(cut):
    """zf -> zi.  Each piece equals IirStage + DacStage on that piece bit for bit.  Against the row filtered whole the
    two pieces are another execution form of one arithmetic (a cut moves the places where lane runs start): for rows of
    first-order sections tests/test_gpu_iir_rows.py::test_two_pieces_equal_the_whole holds y to 1e-12 * scale, so a
    code may differ only where the whole row's v lies within |gain| * 1e-12 * scale of a half-integer -- of 36000
    samples at 1e-8 LSB none is expected, the test asserts there is none and then that the codes are equal"""
    n, batch = 12000, 3
    case = ref.Case(3, 1, batch, n)
    whole = fused(case.rows, case.x, case.gain, case.offset, initial=case.initial, zi=case.zi)
    iir = distortion.IirStage(case.rows, n, batch)
    y = iir.apply_torch(to_dev(case.x), out=torch.empty((batch, n), dtype=torch.float64, device=dev()),
                        initial=case.initial, zi=to_dev(case.zi)).cpu().numpy()
    iir.close()
    v = y * case.gain[:, None] + case.offset[:, None]
    delta = np.abs(case.gain)[:, None] * 1e-12 * max(1.0, np.abs(y).max()) + 2.0**-50 * np.maximum(1.0, np.abs(v))
    assert not np.any(np.abs(v - np.floor(v) - 0.5) <= delta)
    first = fused(case.rows, case.x[:, :cut], case.gain, case.offset, initial=case.initial, zi=case.zi)
    second = fused(case.rows, case.x[:, cut:], case.gain, case.offset, initial=case.initial, zi=first[2])
    ref1 = two_launches(case.rows, case.x[:, :cut], case.gain, case.offset, initial=case.initial, zi=case.zi)
    ref2 = two_launches(case.rows, case.x[:, cut:], case.gain, case.offset, initial=case.initial, zi=ref1[2])
    for i, name in enumerate(('codes', 'counts', 'zf')):
        same(first[i], ref1[i], f'first piece, {name}')
        same(second[i], ref2[i], f'second piece, {name}')
    same(np.hstack([first[0], second[0]]), whole[0], 'the two pieces against the whole')
    same(first[1] + second[1], whole[1], 'counts of the two pieces against the whole')
    assert np.abs(second[2] - whole[2]).max() <= 1e-12 * max(1.0, np.abs(whole[2]).max())


# ---- shared input --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_shared_input_equals_a_broadcast_input(kind):
    n, batch = TILE + 77, 5
    case = ref.Case(1, 2, batch, n, dtype=NP_OF[kind])
    one = case.x[:1]
    st = distortion.IirDacStage(case.rows, n, case.gain, offset=case.offset, dtype=NP_OF[kind])
    spread = fused(None, np.repeat(one, batch, axis=0), None, None, initial=case.initial, zi=case.zi, stage=st)
    for x in (to_dev(one), to_dev(one[0])):                               # (1, n) and 1-D
        zf = torch.empty((batch, st.state_dim), dtype=torch.float64, device=dev())
        c = torch.full((batch, 3), -3, dtype=torch.int64, device=dev())
        y = st.apply_torch(x, counts=c, initial=case.initial, zi=to_dev(case.zi), zf=zf)
        same(y.cpu().numpy(), spread[0], 'shared input, codes')
        same(c.cpu().numpy(), spread[1], 'shared input, counts')
        same(zf.cpu().numpy(), spread[2], 'shared input, zf')
    # codes that meet the one row are refused
    buf = torch.zeros(4 * n, dtype=TORCH_OF[kind], device=dev())
    with pytest.raises(ValueError, match='out of place'):
        st.apply_torch(buf[:n], buf.view(torch.int16)[:batch * n].view(batch, n))
    st.close()


# ---- graph replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_graph_replay_equals_eager(kind):
    """one apply captured (no allocation, no synchronisation inside it: the capture would refuse) and replayed on fresh
    feeds: codes, counts and zf are those of an eager apply of a twin stage on the same feed and of the two launches;
    the counts are overwritten by every replay, not added to"""
    n, batch = TILE + 3, 3
    case = ref.Case(1, 3, batch, n, 14, 2, dtype=NP_OF[kind])
    make = lambda: distortion.IirDacStage(case.rows, n, case.gain, offset=case.offset, bits=14, shift=2, dtype=NP_OF[kind])
    st, twin = make(), make()
    x = torch.empty((batch, n), dtype=TORCH_OF[kind], device=dev())
    out = torch.empty((batch, n), dtype=torch.int16, device=dev())
    counts = torch.empty((batch, 3), dtype=torch.int64, device=dev())
    zf = torch.empty((batch, st.state_dim), dtype=torch.float64, device=dev())
    lv, zi = to_dev(case.initial), to_dev(case.zi)
    feeds = [[case.x], [ref.Case(1, 3, batch, n, seed=4242, dtype=NP_OF[kind]).x * 1.5]]
    got = graph_replay.replay(lambda: st.apply_torch(x, out, counts, initial=lv, zi=zi, zf=zf), [x], feeds,
                              [out, counts, zf])
    for i, feed in enumerate(feeds):
        want = two_launches(case.rows, feed[0], case.gain, case.offset, 14, 2, case.initial, case.zi)
        eager = graph_replay.eager(lambda: twin.apply_torch(x, out, counts, initial=lv, zi=zi, zf=zf), [x], feed,
                                   [out, counts, zf])
        for j, name in enumerate(('codes', 'counts', 'zf')):
            same(got[i][j], want[j], f'replay {i} {name} {kind}')
            same(eager[j], got[i][j], f'eager {i} {name} {kind}')
        assert want[1][:, :2].any()
    st.close()
    twin.close()


# ---- the sampler in front: SampledIirDac -----------------------------------------------------------------------------------
N_AWG, N_FINE = 12000, 12001                             # two whole tiles and a part, as tests/test_gpu_iir_rows_chain.py
TCS = [[(0.02, 150e-9)], [(-0.02, 80e-9), (-0.01, 1.5e-6)], [(0.03, 40e-9), (0.01, 900e-9), (-0.005, 5e-6)]]
LEVELS = np.array([0.0, 0.3, -0.2])
SAMPLED_NAME = {'lean': 'iir_rows_sampled_dac<f64,3,1>', 'short': 'iir_rows_short_dac<f64,3,1>'}


def sampled_config(path):
    """-> (channels, grid, one cascade per row): a fine grid (the lean fill), AWG-rate pieces (the short fill), a clipped
    channel on the fine grid (no fill takes it)"""
    import waveforms_amd as wf
    from waveforms_amd import workloads as wl
    secs = [[distortion.exp_decay_filter(A, tau, 2e9) for A, tau in tc] for tc in TCS]
    if path == 'short':
        return [wl.awg_channel(wf, c, N_AWG, 2e9) for c in range(3)], wl.awg_grid(N_AWG, 2e9), secs
    chans = [wl.sum_channel(wf, 6, 1000 + c) for c in range(3)]
    if path == 'unfusable':
        chans[1].max, chans[1].min = 0.4, -0.3
    return chans, ('linspace', 0.0, 6 * wl.SPAN, N_FINE, False), secs


def sampled_two_launches(chans, grid, secs, gain, offset, bits, shift):
    """SampledIirRows, then DacStage -> (codes, counts, zf, the filtered rows)"""
    sr = distortion.SampledIirRows(chans, grid, secs)
    dac = distortion.DacStage(gain, sr.n, offset=offset, bits=bits, shift=shift, batch=sr.n_channels)
    try:
        z = torch.empty((sr.n_channels, sr.n), dtype=torch.float64, device=dev())
        zf = torch.empty((sr.n_channels, sr.state_dim), dtype=torch.float64, device=dev())
        c = torch.full((sr.n_channels, 3), -1, dtype=torch.int64, device=dev())
        sr.launch_torch(z, initial=LEVELS, zf=zf)
        y = dac.apply_torch(z, counts=c)
        return y.cpu().numpy(), c.cpu().numpy(), zf.cpu().numpy(), z.cpu().numpy(), sr.fused, sr.kernel_name()
    finally:
        sr.close()
        dac.close()


@pytest.mark.parametrize('path', ['lean', 'short', 'unfusable'])
def test_sampled_codes_counts_and_zf_equal_sampled_rows_then_dac(path):
    chans, grid, secs = sampled_config(path)
    bits, shift = 14, 2
    probe = sampled_two_launches(chans, grid, secs, 1.0, 0.0, bits, shift)
    gain, offset = ref.gains_offsets(probe[3], bits, 77)                 # both signs, both rails, fractional offsets
    want = sampled_two_launches(chans, grid, secs, gain, offset, bits, shift)
    sd = distortion.SampledIirDac(chans, grid, secs, gain, offset=offset, bits=bits, shift=shift)
    assert sd.fused == want[4] == (path != 'unfusable'), (sd.why_not, want[5])
    if sd.fused:
        assert sd.kernel_name() == SAMPLED_NAME[path] and sd.why_not == '' and want[5] == SAMPLED_NAME[path].replace('_dac', '')
    else:
        assert 'clip' in sd.why_not and 'scratch' in sd.why_not
        assert sd.kernel_name().endswith(' + iir_rows_dac<f64,3,1>') and not sd.kernel_name().startswith('iir_rows')
    n, rows = sd.n, sd.n_channels
    win = Window(rows, n, np.int16)
    counts = torch.full((rows, 3), 0x5a5a5a5a5a, dtype=torch.int64, device=dev())
    zf = torch.full((rows, sd.state_dim), 9.0, dtype=torch.float64, device=dev())
    assert sd.launch_torch(win.win, counts=counts, initial=LEVELS, zf=zf).data_ptr() == win.ptr
    torch.cuda.synchronize()
    same(win.host(), want[0], f'{path}: codes')
    same(counts.cpu().numpy(), want[1], f'{path}: counts')
    same(zf.cpu().numpy(), want[2], f'{path}: zf')
    win.assert_guards()
    assert (want[1][:, 0] > 0).all() and (want[1][:, 1] > 0).all()
    # the host round trip, and a second launch into the same tensors
    codes, c2, z2 = sd.to_host(initial=LEVELS, return_counts=True, return_zf=True)
    same(codes, want[0], f'{path}: to_host codes')
    same(c2, want[1], f'{path}: to_host counts')
    same(z2, want[2], f'{path}: to_host zf')
    same(sd.to_host(initial=LEVELS), want[0], f'{path}: to_host, codes alone')
    inside = -(-(win.wide.stride(0) + 5) // 4) * 4                      # an int64 boundary inside the first code row
    with pytest.raises(ValueError, match='counts overlaps codes'):
        sd.launch_torch(win.win, counts=win.wide.view(-1)[inside:inside + rows * 12].view(torch.int64).view(rows, 3))
    sd.close()


@pytest.mark.parametrize('path', ['lean', 'short'])
def test_sampled_unfused_switch_gives_the_same_codes(path):
    chans, grid, secs = sampled_config(path)
    gain, offset = ref.gains_offsets(sampled_two_launches(chans, grid, secs, 1.0, 0.0, 16, 0)[3], 16, 78)
    sd = distortion.SampledIirDac(chans, grid, secs, gain, offset=offset)
    assert sd.fused and sd.kernel_name() == SAMPLED_NAME[path]
    fused_out = sd.to_host(initial=LEVELS, return_counts=True, return_zf=True)
    sd.close()
    os.environ['WFK_CHAIN_UNFUSED'] = '1'
    try:
        su = distortion.SampledIirDac(chans, grid, secs, gain, offset=offset)
        assert not su.fused and 'WFK_CHAIN_UNFUSED' in su.why_not and su.kernel_name().endswith(' + iir_rows_dac<f64,3,1>')
        unfused_out = su.to_host(initial=LEVELS, return_counts=True, return_zf=True)
        su.close()
    finally:
        del os.environ['WFK_CHAIN_UNFUSED']
    # (the fill inside the tile and the sampler's own kernel are two execution forms of the sampler's arithmetic, a few
    #  ulp of a sample apart -- tests/test_gpu_iir_rows_chain.py holds them to FP64_IIR_TOL: the codes and counts of these
    #  rows are the same, the final states agree to that tolerance)
    same(fused_out[0], unfused_out[0], f'{path}: fused against WFK_CHAIN_UNFUSED=1, codes')
    same(fused_out[1], unfused_out[1], f'{path}: fused against WFK_CHAIN_UNFUSED=1, counts')
    assert np.abs(fused_out[2] - unfused_out[2]).max() <= FP64_IIR_TOL * max(1.0, np.abs(unfused_out[2]).max())
    assert fused_out[1][:, :2].any()


@pytest.mark.parametrize('path', ['short', 'unfusable'])
def test_sampled_graph_replay_equals_eager(path):
    """a launch captured and replayed: no allocation, no synchronisation (the scratch of the unfused route was taken at
    construction), the counts overwritten by every replay"""
    chans, grid, secs = sampled_config(path)
    gain, offset = np.array([20000.0, -30000.0, 25000.0]), np.array([0.25, -0.5, 100.125])
    sd = distortion.SampledIirDac(chans, grid, secs, gain, offset=offset)
    twin = distortion.SampledIirDac(chans, grid, secs, gain, offset=offset)
    rows, n = sd.n_channels, sd.n
    out = torch.empty((rows, n), dtype=torch.int16, device=dev())
    counts = torch.empty((rows, 3), dtype=torch.int64, device=dev())
    lv = torch.empty(rows, dtype=torch.float64, device=dev())
    feeds = [[LEVELS], [LEVELS[::-1].copy()]]
    got = graph_replay.replay(lambda: sd.launch_torch(out, counts=counts, initial=lv), [lv], feeds, [out, counts])
    for i, feed in enumerate(feeds):
        eager = graph_replay.eager(lambda: twin.launch_torch(out, counts=counts, initial=lv), [lv], feed, [out, counts])
        same(got[i][0], eager[0], f'{path}: replay {i} codes')
        same(got[i][1], eager[1], f'{path}: replay {i} counts')
        same(got[i][0], twin.to_host(initial=feed[0]), f'{path}: replay {i} against the host round trip')
    assert not np.array_equal(got[0][0], got[1][0])
    sd.close()
    twin.close()


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------
def test_plain_c_consumer_filters_to_codes_on_the_device(tmp_path):
    exe = tmp_path / 'iir_dac_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'iir_dac_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'filtered to codes on the device' in r.stdout and 'codes ok' in r.stdout, r.stdout
