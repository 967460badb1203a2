"""The per-row curve + IIR stage that ends in DAC codes on the device (distortion.CurveIirDacStage / curve_iir_dac_rows,
csrc/wfk_iir_rows_curve_dac.hip) against the two stages it replaces, CurveStage followed by IirDacStage on the same
device -- codes, the converter's counts, the curve's `beyond` and zf bit for bit, no tolerance -- and against the NumPy
referee (tests/curve_iir_dac_ref.py), where `beyond` is exact and a code may differ by one step at an UNDECIDED sample and
nowhere else (that the share of such samples is small is held, from the referee alone, by
tests/test_curve_iir_dac_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import curve_iir_dac_ref as ref
import graph_replay
from row_windows import FarWindow, Window, free_far_arena
from waveforms_amd import _engine, _rows, distortion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_OF = {'f64': np.float64, 'f32': np.float32}
TORCH_OF = {'f64': torch.float64, 'f32': torch.float32}
TILE = ref.TILE
SENTINEL = -21846                                        # 0xAAAA
GARBAGE = 0x5a5a5a5a5a
NAMES = ('codes', 'counts', 'beyond', 'zf')


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}')


def same_all(a, b, what):
    for i, name in enumerate(NAMES):
        same(a[i], b[i], f'{name} {what}')


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Pair:
    """the fused stage and the composition it replaces, built once for a case"""

    def __init__(self, case, curves=None):
        c = self.case = case
        xp, fp = curves or (c.xp, c.fp)
        self.fused = distortion.CurveIirDacStage(xp, fp, c.rows, c.n, c.gain, offset=c.offset, bits=c.bits,
                                                 shift=c.shift, left=c.left, right=c.right, dtype=c.dtype)
        self.curve = distortion.CurveStage(xp, fp, c.n, c.batch, c.left, c.right, c.dtype)
        self.iir_dac = distortion.IirDacStage(c.rows, c.n, c.gain, offset=c.offset, bits=c.bits, shift=c.shift,
                                              dtype=c.dtype)

    def one(self, x, initial=None, zi='case', counts=True, beyond=True):
        """x through the fused stage, the reports from tensors of garbage -> (codes, counts, beyond, zf), None where a
        report was not asked for"""
        c = self.case
        zf = torch.full((c.batch, self.fused.state_dim), 9.0, dtype=torch.float64, device=dev())
        cn = torch.full((c.batch, 3), GARBAGE, dtype=torch.int64, device=dev()) if counts else None
        bn = torch.full((c.batch, 3), -GARBAGE, dtype=torch.int64, device=dev()) if beyond else None
        y = self.fused.apply_torch(to_dev(x), counts=cn, beyond=bn, initial=c.initial if initial is None else initial,
                                   zi=to_dev(c.zi) if isinstance(zi, str) else zi, zf=zf)
        assert y.dtype == torch.int16 and tuple(y.shape) == (c.batch, c.n)
        return (y.cpu().numpy(), cn.cpu().numpy() if counts else None, bn.cpu().numpy() if beyond else None,
                zf.cpu().numpy())

    def two(self, x, initial=None, zi='case'):
        """CurveStage, then IirDacStage -> (codes, counts, beyond, zf)"""
        c = self.case
        zf = torch.full((c.batch, self.iir_dac.state_dim), 9.0, dtype=torch.float64, device=dev())
        cn = torch.full((c.batch, 3), -1, dtype=torch.int64, device=dev())
        bn = torch.full((c.batch, 3), -1, dtype=torch.int64, device=dev())
        v = torch.empty((c.batch, c.n), dtype=_rows.torch_dtype(c.dtype), device=dev())
        self.curve.apply_torch(to_dev(x), out=v, counts=bn)
        y = self.iir_dac.apply_torch(v, counts=cn, initial=c.initial if initial is None else initial,
                                     zi=to_dev(c.zi) if isinstance(zi, str) else zi, zf=zf)
        return y.cpu().numpy(), cn.cpu().numpy(), bn.cpu().numpy(), zf.cpu().numpy()

    def close(self):
        for st in (self.fused, self.curve, self.iir_dac):
            st.close()


# ---- against the two stages: exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('nsec,order', ref.SHAPES)
def test_codes_reports_and_zf_equal_curve_stage_then_iir_dac_stage(nsec, order, kind):
    """every length, batch and format of the referee's lists; ragged curves taken in turn from the pool (K = 2, K = 1024
    -- in float64 with the smaller bucket table -- and the row without buckets among them); left / right defaulted,
    given, and with NaN; gains of both signs that clip rows on both rails, per-row levels, a zi; each case on its finite
    input and on the input with the curve's specials"""
    seen = np.zeros((2, 3), dtype=np.int64)                  # [counts, beyond] x [below, above, nan]
    knots, turn = set(), 0
    for n in ref.LENGTHS:
        for batch in ref.BATCHES:
            for bits, shift in ref.FORMATS:
                turn += 1
                case = ref.Case(nsec, order, batch, n, bits, shift, dtype=NP_OF[kind], first=turn % 7,
                                ends=('default', 'given', 'nan')[turn % 3])
                pair = Pair(case)
                knots |= {len(x) for x in case.xp} | ({'wide'} if any(ref.wide(x) for x in case.xp) else set())
                for flavour, x in (('finite', case.x), ('specials', case.x_special)):
                    what = f'({nsec},{order}) {kind} n={n} batch={batch} bits={bits} shift={shift} {flavour}'
                    a, b = pair.one(x), pair.two(x)
                    same_all(a, b, what)
                    if n >= TILE and flavour == 'specials':
                        assert (a[2] > 0).all(), what                       # below, above and NaN in every row
                    if n >= TILE and flavour == 'finite' and case.left is None:
                        assert (a[1][:, :2] > 0).all(), what                # both rails, every row
                    seen += np.stack([a[1].sum(axis=0), a[2].sum(axis=0)])
                pair.close()
    assert seen.all(), seen
    assert {2, 33, 65, 1024, 'wide'} <= knots


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_kernel_names_and_consistency_of_the_entry_points(kind):
    n = 3001
    for nsec, order in ref.SHAPES:
        case = ref.Case(nsec, order, 2, 16, dtype=NP_OF[kind])
        st = distortion.CurveIirDacStage(case.xp, case.fp, case.rows, 16, 100.0, bits=14, shift=1, dtype=NP_OF[kind])
        assert st.kernel_name() == f'iir_rows_curve_dac<{kind},{nsec},{order}>'
        assert (st.n, st.batch, st.state_dim, st.lo, st.hi, st.bits, st.shift) == (16, 2, nsec * order, -8192, 8191, 14, 1)
        assert st.gain.tolist() == [100.0, 100.0] and st.offset.tolist() == [0.0, 0.0]
        assert st.knots.tolist() == [len(x) for x in case.xp]
        st.close()
    case = ref.Case(1, 3, 3, n, dtype=NP_OF[kind], ends='given')
    got = distortion.curve_iir_dac_rows(case.x_special, case.xp, case.fp, case.rows, case.gain, case.offset,
                                        left=case.left, right=case.right, initial=case.initial, return_counts=True)
    pair = Pair(case)
    want = pair.two(case.x_special, zi=None)                      # (the wrapper starts from a zero state)
    for i in range(3):
        same(got[i], want[i], f'curve_iir_dac_rows {NAMES[i]}')
    same(distortion.curve_iir_dac_rows(case.x_special, case.xp, case.fp, case.rows, case.gain, case.offset, left=case.left,
                                       right=case.right, initial=case.initial), want[0], 'curve_iir_dac_rows, codes alone')
    pair.close()
    # from_full_scale; ONE curve and ONE cascade for every row; the inverse of a measured f(V)
    fs = np.array([0.7, 1.0, 1.3])
    volts = np.linspace(-1.0, 1.0, 41)
    detuning = -3.0 * volts - 0.8 * volts**3                      # descending: inverse_rows reverses it
    xs, fss = distortion.CurveStage.inverse_rows(volts, detuning)
    x = np.random.default_rng(5).uniform(-4.2, 4.2, (3, n)).astype(NP_OF[kind])
    st = distortion.CurveIirDacStage.from_full_scale(xs[0], fss[0], case.rows[0], n, fs, bits=14, shift=2, dtype=NP_OF[kind])
    assert st.batch == 3 and np.array_equal(st.gain, 8191 / fs) and st.knots.tolist() == [41] * 3
    codes = st.apply_torch(to_dev(x)).cpu().numpy()
    st.close()
    inv = distortion.CurveStage.inverse(volts, detuning, n, batch=3, dtype=NP_OF[kind])
    tail = distortion.IirDacStage(case.rows[0], n, 8191 / fs, bits=14, shift=2, dtype=NP_OF[kind])
    same(codes, tail.apply_torch(inv.apply_torch(to_dev(x))).cpu().numpy(), 'from_full_scale on an inverse curve')
    inv.close()
    tail.close()


# ---- against the referee ------------------------------------------------------------------------------------------------
def test_beyond_is_exact_and_codes_differ_from_the_referee_only_at_undecided_samples():
    for case in ref.referee_cases():
        what = f'({case.nsec},{case.order}) n={case.n} bits={case.bits}'
        pair = Pair(case)
        codes, counts, beyond, zf = pair.one(case.x)
        pair.close()
        want, want_counts, want_beyond, want_zf = case.reference()
        same(beyond, want_beyond, f'beyond {what}')
        mask, near_lo, near_hi = case.undecided()
        diff = codes.astype(np.int64) - want.astype(np.int64)
        print(f'{what}: {np.count_nonzero(diff)} codes differ, {int(mask.sum())} undecided')
        assert not diff[~mask].any(), (what, np.argwhere((diff != 0) & ~mask)[:4])
        assert np.all(np.abs(diff) <= 1 << case.shift), what
        cd = np.abs(counts - want_counts)
        assert (cd[:, 0] <= near_lo.sum(axis=1)).all() and (cd[:, 1] <= near_hi.sum(axis=1)).all(), (what, cd)
        assert not counts[:, 2].any()
        scale = np.maximum(1.0, np.abs(want_zf).max(axis=1))
        assert (np.abs(zf - want_zf).max(axis=1) <= 1e-9 * scale).all(), what
    # the curve's specials, the row without buckets included: `beyond` exact, every class counted in every row
    case = ref.Case(1, 1, 7, 2 * TILE + 5, first=0)
    pair = Pair(case)
    got = pair.one(case.x_special)
    pair.close()
    want = case.reference(case.x_special)
    same(got[2], want[2], 'beyond of the specials')
    assert (got[2] > 0).all()
    same(got[1][:, 2], want[1][:, 2], 'NaN codes of the specials')          # a NaN sample poisons the state: exact


# ---- memory and reproducibility ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'f32'])
@pytest.mark.parametrize('n', [5, 1024, TILE + 5])
def test_windows_and_guards(n, kind):
    """both sides as windows at an odd element offset of wider tensors with odd row strides; the guards of both sides
    stay, compared as bits, and the input is bit for bit what was put there"""
    dtype = NP_OF[kind]
    case = ref.Case(1, 3, 5, n, 14, 2, dtype=dtype, first=0)
    pair = Pair(case)
    want = pair.two(case.x_special)
    src, dst = Window(5, n, dtype, case.x_special), Window(5, n, np.int16)
    counts = torch.full((5, 3), -77, dtype=torch.int64, device=dev())
    beyond = torch.full((5, 3), -78, dtype=torch.int64, device=dev())
    zf = torch.empty((5, 3), dtype=torch.float64, device=dev())
    res = pair.fused.apply_torch(src.win, dst.win, counts, beyond, initial=case.initial, zi=to_dev(case.zi), zf=zf)
    assert res.data_ptr() == dst.ptr
    torch.cuda.synchronize()
    same_all((dst.host(), counts.cpu().numpy(), beyond.cpu().numpy(), zf.cpu().numpy()), want, f'window n={n} {kind}')
    dst.assert_guards()
    src.assert_holds(case.x_special)
    pair.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_every_lead_of_a_code_row_into_a_sentinel_filled_tensor(kind):
    """code rows at every lead 0 .. 7 into a 16-byte group: [0, n) of every row is written, the sentinels before, after
    and between the rows stay; a second apply overwrites both reports"""
    dtype = NP_OF[kind]
    for n in (3, 2 * TILE + 9):
        case = ref.Case(2, 1, 3, n, 14, 2, dtype=dtype, first=4)     # codes are multiples of 4: none is the sentinel
        pair = Pair(case)
        want = pair.two(case.x, zi=None)
        assert not np.any(want[0] == SENTINEL)
        x = to_dev(case.x)
        for lead in range(8):
            out = torch.full((3, n + 64), SENTINEL, dtype=torch.int16, device=dev())
            counts = torch.full((3, 3), -77, dtype=torch.int64, device=dev())
            beyond = torch.full((3, 3), -78, dtype=torch.int64, device=dev())
            res = pair.fused.apply_torch(x, out[:, lead:lead + n], counts, beyond, initial=case.initial)
            assert res.data_ptr() == out[:, lead:].data_ptr() and tuple(res.shape) == (3, n)
            full = out.cpu().numpy()
            same(full[:, lead:lead + n], want[0], f'n={n} lead={lead} {kind}')
            assert np.all(full[:, :lead] == SENTINEL) and np.all(full[:, lead + n:] == SENTINEL)
            pair.fused.apply_torch(x, out[:, lead:lead + n], counts, beyond, initial=case.initial)
            same(counts.cpu().numpy(), want[1], f'counts of a second apply n={n} lead={lead} {kind}')
            same(beyond.cpu().numpy(), want[2], f'beyond of a second apply n={n} lead={lead} {kind}')
        pair.close()


@pytest.mark.parametrize('kind,side', [('f64', 'far_in'), ('f64', 'far_out')])
def test_rows_more_than_2_pow_32_elements_apart(kind, side):
    dtype, n = NP_OF[kind], TILE + 3
    case = ref.Case(1, 3, 2, n, dtype=dtype, first=1)
    pair = Pair(case)
    want = pair.two(case.x_special)
    src = dst = None
    try:
        if side == 'far_in':
            src, dst = FarWindow(n, dtype, case.x_special), Window(2, n, np.int16)
        else:
            src, dst = Window(2, n, dtype, case.x_special), FarWindow(n, np.int16)
        assert max(src.stride, dst.stride) > 2**32
        counts = torch.full((2, 3), 5, dtype=torch.int64, device=dev())
        beyond = torch.full((2, 3), 6, dtype=torch.int64, device=dev())
        res = pair.fused.apply_torch(src.win, dst.win, counts, beyond, initial=case.initial, zi=to_dev(case.zi))
        assert res.data_ptr() == dst.ptr
        torch.cuda.synchronize()
        same(dst.host(), want[0], f'far rows {kind} {side}')
        same(counts.cpu().numpy(), want[1], f'far rows counts {kind} {side}')
        same(beyond.cpu().numpy(), want[2], f'far rows beyond {kind} {side}')
        dst.assert_guards()
        src.assert_holds(case.x_special)
    finally:
        pair.close()
        del src, dst
        free_far_arena()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_garbage_in_the_reports_one_report_and_none(kind):
    """both reports from garbage; one given and the other None, either way; neither: the codes and zf are the same"""
    n = 2 * TILE + 100
    case = ref.Case(1, 3, 7, n, dtype=NP_OF[kind], first=0)
    pair = Pair(case)
    want = pair.two(case.x_special)
    both = pair.one(case.x_special)
    same_all(both, want, 'both reports')
    only_counts = pair.one(case.x_special, beyond=False)
    only_beyond = pair.one(case.x_special, counts=False)
    neither = pair.one(case.x_special, counts=False, beyond=False)
    assert only_counts[2] is None and only_beyond[1] is None and neither[1] is None and neither[2] is None
    same(only_counts[1], want[1], 'counts alone')
    same(only_beyond[2], want[2], 'beyond alone')
    for got, name in ((only_counts, 'counts alone'), (only_beyond, 'beyond alone'), (neither, 'no report')):
        same(got[0], want[0], f'codes, {name}')
        same(got[3], want[3], f'zf, {name}')
    assert (want[2] > 0).all()
    pair.close()


@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_permutation_and_repeatability(kind):
    n = 2 * TILE + 100
    case = ref.Case(1, 3, 7, n, dtype=NP_OF[kind], first=0)
    perm = np.random.default_rng(1).permutation(7)
    pair = Pair(case)
    a, b = pair.one(case.x), pair.one(case.x)
    same_all(a, b, 'two runs')
    assert a[1][:, :2].all()
    pc = ref.Case(1, 3, 7, n, dtype=NP_OF[kind], first=0)
    pc.xp, pc.fp = [case.xp[i] for i in perm], [case.fp[i] for i in perm]
    pc.rows, pc.gain, pc.offset = [case.rows[i] for i in perm], case.gain[perm], case.offset[perm]
    pc.initial, pc.zi = case.initial[perm], case.zi[perm]
    pp = Pair(pc)
    p = pp.one(case.x[perm])
    for i, name in enumerate(NAMES):
        same(p[i], a[i][perm], f'permuted rows, {name}')
    pp.close()
    pair.close()


@pytest.mark.parametrize('cut', [TILE + 1234, 2 * TILE])              # inside a tile / on a tile edge
def test_a_row_cut_in_two_equals_the_composition_on_each_piece(cut):
    """zf -> zi: each piece equals CurveStage + IirDacStage on that piece bit for bit, and `beyond` of the two pieces adds
    up to the whole row's"""
    n, batch = 12000, 3
    case = ref.Case(3, 1, batch, n, first=1)
    pair = Pair(case)
    whole = pair.one(case.x)
    pair.close()

    def piece(lo, hi):
        c = ref.Case(3, 1, batch, hi - lo, first=1)
        c.rows, c.gain, c.offset, c.initial, c.zi = case.rows, case.gain, case.offset, case.initial, case.zi
        return Pair(c)

    p1, p2 = piece(0, cut), piece(cut, n)
    first, ref1 = p1.one(case.x[:, :cut]), p1.two(case.x[:, :cut])
    second, ref2 = p2.one(case.x[:, cut:], zi=to_dev(first[3])), p2.two(case.x[:, cut:], zi=to_dev(ref1[3]))
    same_all(first, ref1, 'first piece')
    same_all(second, ref2, 'second piece')
    same(first[2] + second[2], whole[2], 'beyond of the two pieces against the whole')
    assert np.abs(second[3] - whole[3]).max() <= 1e-9 * max(1.0, np.abs(whole[3]).max())
    p1.close()
    p2.close()


# ---- shared input --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_shared_input_equals_a_broadcast_input(kind):
    n, batch = TILE + 77, 5
    case = ref.Case(1, 2, batch, n, dtype=NP_OF[kind], first=1)
    # one row for every curve: samples over the union of the ranges, so that every curve is left on both sides
    one = np.random.default_rng(9).uniform(-1.2, 1.2, (1, n)).astype(NP_OF[kind])
    one[0, 5:8] = [np.nan, np.inf, -np.inf]
    pair = Pair(case)
    spread = pair.one(np.repeat(one, batch, axis=0))
    same_all(spread, pair.two(np.repeat(one, batch, axis=0)), 'broadcast input')
    for x in (to_dev(one), to_dev(one[0])):                               # (1, n) and 1-D
        zf = torch.empty((batch, pair.fused.state_dim), dtype=torch.float64, device=dev())
        c = torch.full((batch, 3), -3, dtype=torch.int64, device=dev())
        b = torch.full((batch, 3), -4, dtype=torch.int64, device=dev())
        y = pair.fused.apply_torch(x, counts=c, beyond=b, initial=case.initial, zi=to_dev(case.zi), zf=zf)
        same_all((y.cpu().numpy(), c.cpu().numpy(), b.cpu().numpy(), zf.cpu().numpy()), spread, 'shared input')
    buf = torch.zeros(4 * n, dtype=TORCH_OF[kind], device=dev())
    with pytest.raises(ValueError, match='out of place'):
        pair.fused.apply_torch(buf[:n], buf.view(torch.int16)[:batch * n].view(batch, n))
    pair.close()


# ---- refusals at both levels -----------------------------------------------------------------------------------------------
def test_overlap_and_refused_tensors():
    n, rows = 256, 3
    case = ref.Case(1, 1, rows, n)
    st = distortion.CurveIirDacStage(case.xp, case.fp, case.rows, n, 1000.0)
    buf = torch.zeros(rows * n + 64, dtype=torch.float64, device=dev())
    x = buf[:rows * n].view(rows, n)
    as_codes = buf.view(torch.int16)                                      # the same bytes as int16
    out = torch.zeros((rows, n), dtype=torch.int16, device=dev())
    reports = torch.zeros((2, rows, 3), dtype=torch.int64, device=dev())
    counts, beyond = reports[0], reports[1]
    st.apply_torch(x, out, counts, beyond)                                # fine
    for bad_out in (as_codes[:rows * n].view(rows, n), as_codes[4 * rows * n - rows * n + 8:][:rows * n].view(rows, n)):
        with pytest.raises(ValueError, match='curve iir dac stage is out of place: codes overlaps x'):
            st.apply_torch(x, bad_out, counts)
    over_x = buf[8:8 + rows * 3].view(torch.int64).view(rows, 3)
    over_out = out.view(-1)[16:16 + rows * 12].view(torch.int64).view(rows, 3)
    for bad in (over_x, over_out):
        with pytest.raises(ValueError, match='curve iir dac stage: counts overlaps x / codes'):
            st.apply_torch(x, out, bad)
        with pytest.raises(ValueError, match='curve iir dac stage: beyond overlaps x / codes'):
            st.apply_torch(x, out, counts, bad)
    straddle = reports.view(-1)[3:3 + rows * 3].view(rows, 3)
    for c, b in ((counts, counts), (counts, straddle), (straddle, beyond)):
        with pytest.raises(ValueError, match='curve iir dac stage: beyond overlaps counts'):
            st.apply_torch(x, out, c, b)
    for bad in (counts[:2], counts.reshape(-1), counts.to(torch.int32), counts.cpu()):
        with pytest.raises(ValueError, match='expected counts'):
            st.apply_torch(x, out, bad)
        with pytest.raises(ValueError, match='expected beyond'):
            st.apply_torch(x, out, None, bad)
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
    reports.fill_(7)
    X, Y, Cn, Bn = xc.data_ptr(), out.data_ptr(), counts.data_ptr(), beyond.data_ptr()
    for args, message in (((None, n, Y, n, None, None), b'null in / out'),
                          ((X, n, None, n, None, None), b'null in / out'),
                          ((X + 4, n, Y, n, None, None), b'not aligned to their element'),
                          ((X, n, Y + 1, n, None, None), b'not aligned to their element'),
                          ((X, n - 1, Y, n, None, None), b'in row stride smaller'),
                          ((X, n, Y, n - 1, None, None), b'out row stride smaller'),
                          ((X, n, X + 8, n, None, None), b'per-row curve IIR dac is out of place: out overlaps in'),
                          ((X, n, Y, n, Cn + 4, None), b'counts are not aligned'),
                          ((X, n, Y, n, X + 16, None), b'counts overlaps in'),
                          ((X, n, Y, n, Y + 8, None), b'counts overlaps out'),
                          ((X, n, Y, n, None, Bn + 4), b'beyond is not aligned'),
                          ((X, n, Y, n, Cn, X + 16), b'beyond overlaps in'),
                          ((X, n, Y, n, None, Y + 8), b'beyond overlaps out'),
                          ((X, n, Y, n, Cn, Cn), b'beyond overlaps counts'),
                          ((X, n, Y, n, Cn, Cn + 8 * (3 * rows - 1)), b'beyond overlaps counts'),
                          ((X, n, Y, n, Bn - 8, Bn), b'beyond overlaps counts')):
        assert lib.wfk_curve_iir_dac_apply(h, *args, None, None, None, None) == -1, args
        text = lib.wfk_last_error()
        assert text.startswith(b'per-row curve IIR dac') and message in text, (args, text)
        with pytest.raises(_engine.EngineError, match=message.decode()):
            st.plan.apply(*args)
    assert lib.wfk_curve_iir_dac_apply_shared_in(h, X, X + 8, n, None, None, None, None, None, None) == -1
    assert b'shared input is out of place: out overlaps in' in lib.wfk_last_error()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL) and np.all(reports.cpu().numpy() == 7)
    st.close()
    # n = 0: no kernel; both reports are zeroed
    empty = distortion.CurveIirDacStage(case.xp, case.fp, case.rows, 0, 1.0)
    e = torch.zeros((rows, 0), dtype=torch.float64, device=dev())
    reports.fill_(5)
    assert tuple(empty.apply_torch(e, counts=counts, beyond=beyond).shape) == (rows, 0)
    assert not reports.cpu().numpy().any()
    reports.fill_(5)
    empty.apply_torch(e, beyond=beyond)
    assert not beyond.cpu().numpy().any() and (counts.cpu().numpy() == 5).all()
    empty.close()


# ---- graph replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f64', 'f32'])
def test_graph_replay_equals_eager(kind):
    """one apply captured (no allocation, no synchronisation, no memset inside it) and replayed on three feeds: codes,
    both reports and zf are those of an eager apply of a twin stage on the same feed and of the composition; the reports
    are overwritten by every replay, not added to"""
    n, batch = TILE + 3, 3
    case = ref.Case(1, 3, batch, n, 14, 2, dtype=NP_OF[kind], first=0)
    pair, twin = Pair(case), Pair(case)
    x = torch.empty((batch, n), dtype=TORCH_OF[kind], device=dev())
    out = torch.empty((batch, n), dtype=torch.int16, device=dev())
    counts = torch.empty((batch, 3), dtype=torch.int64, device=dev())
    beyond = torch.empty((batch, 3), dtype=torch.int64, device=dev())
    zf = torch.empty((batch, pair.fused.state_dim), dtype=torch.float64, device=dev())
    lv, zi = to_dev(case.initial), to_dev(case.zi)
    other = ref.Case(1, 3, batch, n, seed=4242, dtype=NP_OF[kind], first=0)
    feeds = [[case.x_special], [other.x], [(case.x * 1.02).astype(NP_OF[kind])]]
    outs = [out, counts, beyond, zf]
    got = graph_replay.replay(lambda: pair.fused.apply_torch(x, out, counts, beyond, initial=lv, zi=zi, zf=zf), [x],
                              feeds, outs)
    for i, feed in enumerate(feeds):
        want = pair.two(feed[0])
        eager = graph_replay.eager(lambda: twin.fused.apply_torch(x, out, counts, beyond, initial=lv, zi=zi, zf=zf),
                                   [x], feed, outs)
        same_all(got[i], want, f'replay {i} {kind}')
        same_all(eager, got[i], f'eager {i} {kind}')
        assert want[2][:, :2].any()
    assert not np.array_equal(got[0][2], got[1][2]) and not np.array_equal(got[1][1], got[2][1])
    pair.close()
    twin.close()


# ---- the sampler in front: SampledCurveIirDac ---------------------------------------------------------------------------
N_AWG, N_FINE = 12000, 12001                             # two whole tiles and a part, as tests/test_gpu_iir_dac.py
TCS = [[(0.02, 150e-9)], [(-0.02, 80e-9), (-0.01, 1.5e-6)], [(0.03, 40e-9), (0.01, 900e-9), (-0.005, 5e-6)]]
LEVELS = np.array([0.0, 0.3, -0.2])
SAMPLED_NAME = {'lean': 'iir_rows_sampled_curve_dac<f64,3,1>', 'short': 'iir_rows_short_curve_dac<f64,3,1>'}
IDENTITY = [[([1.0, 0.0], [1.0, 0.0])] * 3] * 3         # all-identity cascades of the shape (3, 1): y = x exactly


def sampled_config(path):
    """-> (channels, grid, one cascade per row): a fine grid (the lean fill), AWG-rate pieces (the short fill), a clipped
    channel on the fine grid (no fill takes it)  (tests/test_gpu_iir_dac.py::sampled_config, copied)"""
    import waveforms_amd as wf
    from waveforms_amd import workloads as wl
    secs = [[distortion.exp_decay_filter(A, tau, 2e9) for A, tau in tc] for tc in TCS]
    if path == 'short':
        return [wl.awg_channel(wf, c, N_AWG, 2e9) for c in range(3)], wl.awg_grid(N_AWG, 2e9), secs
    chans = [wl.sum_channel(wf, 6, 1000 + c) for c in range(3)]
    if path == 'unfusable':
        chans[1].max, chans[1].min = 0.4, -0.3
    return chans, ('linspace', 0.0, 6 * wl.SPAN, N_FINE, False), secs


def sampled_rows(chans, grid):
    """what the sampler's own kernels write: BatchSampler's float64 rows, on the host"""
    from waveforms_amd._sampling import BatchSampler
    bs = BatchSampler(chans, grid)
    try:
        return bs.to_host(np.float64)
    finally:
        bs.close()


def fill_rows(chans, grid):
    """the samples X the FILL produces: SampledIirRows with all-identity cascades of the shape (3, 1) and initial = 0 --
    every state stays +-0 and y = x exactly for finite x, in iir_cascade_step as in the scan"""
    sr = distortion.SampledIirRows(chans, grid, IDENTITY)
    try:
        assert sr.fused and sr.kernel_name() in ('iir_rows_sampled<f64,3,1>', 'iir_rows_short<f64,3,1>')
        z = torch.empty((sr.n_channels, sr.n), dtype=torch.float64, device=dev())
        sr.launch_torch(z, initial=0.0)
        return z.cpu().numpy()
    finally:
        sr.close()


def curves_over(X, K=(33, 128, 500), margin=0.08):
    """one monotone curve per row over the row's range less a margin at each end, so that samples fall beyond on both
    sides; volts of order one"""
    xs, fs = [], []
    for r, k in enumerate(K):
        lo, hi = X[r].min(), X[r].max()
        w = hi - lo
        xp = np.linspace(lo + margin * w, hi - margin * w, k)
        u = np.linspace(-1.0, 1.0, k)
        xs.append(xp)
        fs.append((0.8 + 0.1 * r) * (u + 0.25 * u**3) + 0.05 * r)
    return xs, fs


def composed(X, xs, fs, secs, gain, offset, bits, shift, left=None, right=None):
    """CurveStage in place on X, then IirDacStage, on the device -> (codes, counts, beyond, zf, the filtered volts)"""
    rows, n = X.shape
    curve = distortion.CurveStage(xs, fs, n, rows, left, right)
    tail = distortion.IirDacStage(secs, n, gain, offset=offset, bits=bits, shift=shift)
    iir = distortion.IirStage(secs, n, rows)
    try:
        v = to_dev(X)
        beyond = torch.full((rows, 3), -1, dtype=torch.int64, device=dev())
        counts = torch.full((rows, 3), -1, dtype=torch.int64, device=dev())
        zf = torch.empty((rows, tail.state_dim), dtype=torch.float64, device=dev())
        curve.apply_torch(v, out=v, counts=beyond)
        codes = tail.apply_torch(v, counts=counts, initial=LEVELS, zf=zf)
        y = iir.apply_torch(v, out=torch.empty_like(v), initial=LEVELS)
        return codes.cpu().numpy(), counts.cpu().numpy(), beyond.cpu().numpy(), zf.cpu().numpy(), y.cpu().numpy()
    finally:
        for st in (curve, tail, iir):
            st.close()


@pytest.mark.parametrize('path', ['lean', 'short', 'unfusable'])
def test_sampled_codes_reports_and_zf_equal_the_composition(path):
    """fused: on the fill's own samples X (read out through identity cascades) the result equals CurveStage +
    IirDacStage bit for bit; unfusable: bit for bit against BatchSampler -> CurveStage in place -> IirDacStage"""
    chans, grid, secs = sampled_config(path)
    bits, shift = 14, 2
    X = sampled_rows(chans, grid) if path == 'unfusable' else fill_rows(chans, grid)
    xs, fs = curves_over(X)
    right = np.array([1.1, 1.2, 1.3])                                    # `right` given, `left` defaulted
    probe = composed(X, xs, fs, secs, 1.0, 0.0, bits, shift)
    gain, offset = ref.gains_offsets(probe[4], bits, 77)                 # both signs, both rails, fractional offsets
    want = composed(X, xs, fs, secs, gain, offset, bits, shift, right=right)
    sd = distortion.SampledCurveIirDac(chans, grid, xs, fs, secs, gain, offset=offset, bits=bits, shift=shift, right=right)
    assert sd.fused == (path != 'unfusable'), sd.why_not
    if sd.fused:
        assert sd.kernel_name() == SAMPLED_NAME[path] and sd.why_not == ''
    else:
        assert 'clip' in sd.why_not and 'scratch' in sd.why_not
        assert sd.kernel_name().endswith(' + iir_rows_curve_dac<f64,3,1>') and not sd.kernel_name().startswith('iir_rows')
    n, rows = sd.n, sd.n_channels
    assert sd.knots.tolist() == [33, 128, 500] and sd.plan.table_bytes() > 0
    win = Window(rows, n, np.int16)
    counts = torch.full((rows, 3), GARBAGE, dtype=torch.int64, device=dev())
    beyond = torch.full((rows, 3), -GARBAGE, dtype=torch.int64, device=dev())
    zf = torch.full((rows, sd.state_dim), 9.0, dtype=torch.float64, device=dev())
    assert sd.launch_torch(win.win, counts=counts, beyond=beyond, initial=LEVELS, zf=zf).data_ptr() == win.ptr
    torch.cuda.synchronize()
    got = (win.host(), counts.cpu().numpy(), beyond.cpu().numpy(), zf.cpu().numpy())
    same_all(got, want, path)
    win.assert_guards()
    assert (want[1][:, :2] > 0).all() and (want[2][:, :2] > 0).all() and not want[2][:, 2].any()
    # the host round trip, one report at a time and none
    codes, c2, b2, z2 = sd.to_host(initial=LEVELS, return_counts=True, return_beyond=True, return_zf=True)
    same_all((codes, c2, b2, z2), want, f'{path}: to_host')
    same(sd.to_host(initial=LEVELS), want[0], f'{path}: to_host, codes alone')
    codes, b2 = sd.to_host(initial=LEVELS, return_beyond=True)
    same(codes, want[0], f'{path}: to_host with beyond alone, codes')
    same(b2, want[2], f'{path}: to_host with beyond alone')
    inside = -(-(win.wide.stride(0) + 5) // 4) * 4                      # an int64 boundary inside the first code row
    over = win.wide.view(-1)[inside:inside + rows * 12].view(torch.int64).view(rows, 3)
    with pytest.raises(ValueError, match='counts overlaps codes'):
        sd.launch_torch(win.win, counts=over)
    with pytest.raises(ValueError, match='beyond overlaps codes'):
        sd.launch_torch(win.win, beyond=over)
    with pytest.raises(ValueError, match='beyond overlaps counts'):
        sd.launch_torch(win.win, counts=counts, beyond=counts)
    sd.close()


def test_sampled_lean_curve_too_large_for_the_fill_takes_the_composed_route():
    """1024 knots do not fit next to the lean fill's parameter area: the plan says so and runs the sampler, then
    iir_rows_curve_dac -- bit for bit the composition on the sampler's rows"""
    chans, grid, secs = sampled_config('lean')
    X = sampled_rows(chans, grid)
    xs, fs = curves_over(X, K=(33, 1024, 500))
    gain, offset = np.array([9000.0, -11000.0, 8000.0]), np.array([0.25, -0.5, 100.125])
    want = composed(X, xs, fs, secs, gain, offset, 16, 0)
    sd = distortion.SampledCurveIirDac(chans, grid, xs, fs, secs, gain, offset=offset)
    assert not sd.fused and '1024 knots' in sd.why_not and 'scratch' in sd.why_not
    assert sd.kernel_name().endswith(' + iir_rows_curve_dac<f64,3,1>')
    got = sd.to_host(initial=LEVELS, return_counts=True, return_beyond=True, return_zf=True)
    same_all(got, want, 'a curve too large for the lean fill')
    sd.close()


@pytest.mark.parametrize('path', ['lean', 'short'])
def test_sampled_unfused_switch_gives_the_same_codes(path):
    """(10 bits, left-justified: at |gain| max|slope| FP64_IIR_TOL = 4e-7 LSB the first condition is expected to miss
    0.03 samples of these 36000; at 16 bits it would miss two)"""
    from cases import FP64_IIR_TOL
    bits, shift = 10, 6
    chans, grid, secs = sampled_config(path)
    X = sampled_rows(chans, grid)
    xs, fs = curves_over(X)
    probe = composed(X, xs, fs, secs, 1.0, 0.0, bits, shift)
    gain, offset = ref.gains_offsets(probe[4], bits, 78)
    # two conditions, from the composition on the sampler's own rows: no sample's v within |gain| max|slope| tol scale
    # of a half-integer, no sampled value within tol scale of an end knot
    scale = max(1.0, np.abs(X).max())
    slope = np.array([np.abs(np.diff(f) / np.diff(x)).max() for x, f in zip(xs, fs)])
    v = probe[4] * gain[:, None] + offset[:, None]
    delta = (np.abs(gain) * slope)[:, None] * FP64_IIR_TOL * scale + 2.0**-50 * np.maximum(1.0, np.abs(v))
    assert not np.any(np.abs(v - np.floor(v) - 0.5) <= delta)
    for r in range(3):
        assert not np.any(np.abs(X[r] - xs[r][0]) <= FP64_IIR_TOL * scale)
        assert not np.any(np.abs(X[r] - xs[r][-1]) <= FP64_IIR_TOL * scale)
    sd = distortion.SampledCurveIirDac(chans, grid, xs, fs, secs, gain, offset=offset, bits=bits, shift=shift)
    assert sd.fused and sd.kernel_name() == SAMPLED_NAME[path]
    fused_out = sd.to_host(initial=LEVELS, return_counts=True, return_beyond=True, return_zf=True)
    sd.close()
    os.environ['WFK_CHAIN_UNFUSED'] = '1'
    try:
        su = distortion.SampledCurveIirDac(chans, grid, xs, fs, secs, gain, offset=offset, bits=bits, shift=shift)
        assert not su.fused and 'WFK_CHAIN_UNFUSED' in su.why_not
        assert su.kernel_name().endswith(' + iir_rows_curve_dac<f64,3,1>')
        unfused_out = su.to_host(initial=LEVELS, return_counts=True, return_beyond=True, return_zf=True)
        su.close()
    finally:
        del os.environ['WFK_CHAIN_UNFUSED']
    for i in range(3):
        same(fused_out[i], unfused_out[i], f'{path}: fused against WFK_CHAIN_UNFUSED=1, {NAMES[i]}')
    tol = FP64_IIR_TOL * max(1.0, slope.max())
    assert np.abs(fused_out[3] - unfused_out[3]).max() <= tol * max(1.0, np.abs(unfused_out[3]).max())
    assert fused_out[1][:, :2].any() and fused_out[2][:, :2].all()


@pytest.mark.parametrize('path', ['short', 'unfusable'])
def test_sampled_graph_replay_equals_eager(path):
    """a launch captured and replayed on three feeds (the rows' levels): no allocation, no synchronisation (the scratch
    of the unfused route was taken at construction), both reports overwritten by every replay"""
    chans, grid, secs = sampled_config(path)
    X = sampled_rows(chans, grid)
    xs, fs = curves_over(X)
    gain, offset = np.array([20000.0, -30000.0, 25000.0]), np.array([0.25, -0.5, 100.125])
    sd = distortion.SampledCurveIirDac(chans, grid, xs, fs, secs, gain, offset=offset)
    twin = distortion.SampledCurveIirDac(chans, grid, xs, fs, secs, gain, offset=offset)
    assert sd.fused == (path == 'short')
    rows, n = sd.n_channels, sd.n
    out = torch.empty((rows, n), dtype=torch.int16, device=dev())
    counts = torch.empty((rows, 3), dtype=torch.int64, device=dev())
    beyond = torch.empty((rows, 3), dtype=torch.int64, device=dev())
    lv = torch.empty(rows, dtype=torch.float64, device=dev())
    feeds = [[LEVELS], [LEVELS[::-1].copy()], [LEVELS * 0.5]]
    outs = [out, counts, beyond]
    got = graph_replay.replay(lambda: sd.launch_torch(out, counts=counts, beyond=beyond, initial=lv), [lv], feeds, outs)
    for i, feed in enumerate(feeds):
        eager = graph_replay.eager(lambda: twin.launch_torch(out, counts=counts, beyond=beyond, initial=lv), [lv], feed,
                                   outs)
        host = twin.to_host(initial=feed[0], return_counts=True, return_beyond=True)
        for j in range(3):
            same(got[i][j], eager[j], f'{path}: replay {i} {NAMES[j]}')
            same(got[i][j], host[j], f'{path}: replay {i} against the host round trip, {NAMES[j]}')
        assert got[i][2][:, :2].all()
    assert not np.array_equal(got[0][0], got[1][0])
    if path == 'unfusable':                                # ... and the composition on the sampler's rows
        want = composed(X, xs, fs, secs, gain, offset, 16, 0)
        for j in range(3):
            same(got[0][j], want[j], f'unfusable: replay 0 against the composition, {NAMES[j]}')
    sd.close()
    twin.close()


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------
def test_plain_c_consumer_looks_up_filters_and_converts_on_the_device(tmp_path):
    exe = tmp_path / 'curve_iir_dac_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'curve_iir_dac_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'curve and filter to codes on the device' in r.stdout and 'codes ok' in r.stdout, r.stdout
