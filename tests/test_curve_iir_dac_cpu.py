"""The per-row curve + IIR stage that ends in DAC codes (distortion.CurveIirDacStage / curve_iir_dac_rows,
csrc/wfk_iir_rows_curve_dac.hip) without a device: the referee (tests/curve_iir_dac_ref.py) against np.interp -> scipy ->
dac_ref, the condition the GPU test's comparison with the referee rests on (the undecided share of each of its inputs,
from the referee alone), every refusal before any device work -- the no-device argument check, the stage, the C entry
through ctypes, the curve's first, then the converter's, then the cascade's -- and the symbols with what they return for
a NULL plan."""
import ctypes as C

import numpy as np
import pytest
from scipy.signal import lfilter

import curve_iir_dac_ref as ref
import dac_rows_ref
from waveforms_amd import _engine, distortion

ONE = [[([0.5, 0.25], [1.0, -0.5])]] * 3        # three rows, one first-order section each
XP = [np.array([-1.0, 0.0, 2.0])] * 3
FP = [np.array([-0.5, 0.0, 0.4])] * 3


# ---- the referee -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ends', ['default', 'given'])
def test_referee_is_interp_then_scipy_then_dac_ref(ends):
    case = ref.Case(2, 1, 7, 300, 14, 2, ends=ends)               # seven rows: every curve of the pool
    assert len({len(x) for x in case.xp}) >= 4 and any(ref.wide(x) for x in case.xp)
    codes, counts, beyond, zf = case.reference()
    for r in range(case.batch):
        left = None if case.left is None else case.left[r]
        right = None if case.right is None else case.right[r]
        v = np.interp(case.x[r], case.xp[r], case.fp[r], left, right)
        assert np.array_equal(v, case.v[r])
        y, pos, zs = v - case.initial[r], 0, []
        for b, a in case.rows[r]:
            m = max(len(a), len(b)) - 1
            y, z = lfilter(b, a, y, zi=case.zi[r][pos:pos + m])
            zs.append(z)
            pos += m
        y = y + case.initial[r]
        assert np.array_equal(y, case.y[r]) and np.array_equal(np.concatenate(zs), zf[r])
        want, want_counts = dac_rows_ref.dac_ref(y[None, :], case.gain[r:r + 1], case.offset[r:r + 1], 14, 2)
        assert np.array_equal(want[0], codes[r]) and np.array_equal(want_counts[0], counts[r])
        assert beyond[r].tolist() == [np.count_nonzero(case.x[r] < case.xp[r][0]),
                                      np.count_nonzero(case.x[r] > case.xp[r][-1]), 0]


def test_inputs_reach_every_counter_and_the_specials_poison_as_the_stages_do():
    case = ref.Case(1, 2, 7, ref.TILE + 1)
    codes, counts, beyond, _ = case.reference()
    finite_rows = [r for r in range(7) if not ref.wide(case.xp[r])]
    assert (beyond[finite_rows, :2] > 0).all() and not beyond[:, 2].any()       # beyond both ends, never NaN
    assert (counts[:, :2] > 0).all() and not counts[:, 2].any()                  # both rails, every row
    _, counts_s, beyond_s, _ = case.reference(case.x_special)
    assert (beyond_s > 0).all()                                                  # below, above and NaN in every row
    assert (counts_s[:, 2] > 0).all()                                            # a NaN stays in the state: NaN codes
    assert np.isfinite(case.x).all() and case.x.dtype == np.float64
    # an identical float32 case: the curve's result is rounded to float once before the cascade reads it
    c32 = ref.Case(1, 2, 3, 64, dtype=np.float32)
    assert c32.x.dtype == c32.v.dtype == np.float32 and c32.y.dtype == np.float64


def test_undecided_share_of_the_gpu_tests_inputs():
    for case in ref.referee_cases():
        assert not any(ref.wide(x) for x in case.xp) and np.isfinite(case.y).all()
        tol = case.tol_y()
        mask, near_lo, near_hi = case.undecided(tol)
        share = mask.mean(axis=1)
        delta = np.abs(case.gain) * tol
        print(f'shape ({case.nsec}, {case.order}) n {case.n} bits {case.bits} knots {[len(x) for x in case.xp]}: tol_y '
              f'{tol.max():.3g}, delta {delta.max():.3g} LSB, undecided {int(mask.sum())} (share {share.max():.3g}), at '
              f'the rails {int(near_lo.sum())} / {int(near_hi.sum())}')
        assert (share <= ref.MAX_UNDECIDED_SHARE).all(), (case.nsec, case.order, case.n, case.bits, share)
        _, counts, beyond, _ = case.reference()
        assert (counts[:, :2] > 0).all() and (beyond[:, :2] > 0).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------
OK = dict(xp=XP, fp=FP, rows=ONE, n=8, gain=1000.0, offset=0.0, bits=16, shift=0, dtype=np.float64, left=None, right=None)
BAD = [   # (what differs from OK, exception, message): the curve's, the converter's, the cascade's
    (dict(xp=[np.array([0.0])] * 3, fp=[np.array([0.0])] * 3), ValueError, 'row 0: fewer than 2 knots'),
    (dict(xp=[np.arange(1025.0)] * 3, fp=[np.arange(1025.0)] * 3), ValueError, 'row 0: more than 1024 knots'),
    (dict(xp=XP[:2] + [np.array([-1.0, np.inf, 2.0])]), ValueError, 'row 2: knot 1 is not finite'),
    (dict(xp=XP[:1] + [np.array([-1.0, -1.0, 2.0])] + XP[:1]), ValueError,
     'row 1: knots are not strictly increasing at 1'),
    (dict(fp=FP[:2] + [np.array([0.0, np.nan, 1.0])]), ValueError, 'row 2: value 1 is not finite'),
    (dict(fp=FP[:2] + [np.array([0.0, 1.0])]), ValueError, 'row 2: 3 knots and 2 values'),
    (dict(fp=FP[:2]), ValueError, '3 rows of xp and 2 rows of fp'),
    (dict(left=[0.0, 1.0]), ValueError, '2 values of left for 3 rows'),
    (dict(n=-1), ValueError, 'n >= 0'),
    (dict(dtype=np.int16), ValueError, 'dtype must be float64 or float32'),
    (dict(dtype=np.complex128), NotImplementedError, 'complex'),
    (dict(bits=1), ValueError, r'bits must lie in \[2, 16\]'),
    (dict(bits=17), ValueError, r'bits must lie in \[2, 16\]'),
    (dict(bits=16, shift=1), ValueError, r'shift must lie in \[0, 16 - bits\]'),
    (dict(gain=[1.0, np.inf, 1.0]), ValueError, 'row 1: gain is not finite'),
    (dict(offset=[0.0, 0.0, np.nan]), ValueError, 'row 2: offset is not finite'),
    # the curve's refusal comes before the converter's, the converter's before the cascade's
    (dict(xp=[np.array([0.0])] * 3, fp=[np.array([0.0])] * 3, bits=1), ValueError, 'row 0: fewer than 2 knots'),
    (dict(bits=1, rows=[[]] * 3), ValueError, r'bits must lie in \[2, 16\]'),
    (dict(rows=[[([1.0, 0.5j], [1.0, -0.5])]] * 3), NotImplementedError, 'complex coefficients'),
    (dict(rows=[[]] * 3), ValueError, 'a row without sections'),
]
IDS = [f'{i}-{b[2][:24]}' for i, b in enumerate(BAD)]


@pytest.mark.parametrize('change,exc,message', BAD, ids=IDS)
def test_arguments_refuse_without_a_device(change, exc, message):
    a = dict(OK, **change)
    with pytest.raises(exc, match=message):
        _engine.curve_iir_dac_arguments(a['xp'], a['fp'], a['rows'], np.broadcast_to(a['gain'], 3) if np.ndim(a['gain']) == 0
                                        else a['gain'], np.broadcast_to(a['offset'], 3) if np.ndim(a['offset']) == 0
                                        else a['offset'], a['n'], a['bits'], a['shift'], a['left'], a['right'], None,
                                        a['dtype'])


def test_arguments_count_rows_by_the_curves():
    g = np.ones(3)
    with pytest.raises(ValueError, match='2 gains for 3 rows'):
        _engine.curve_iir_dac_arguments(XP, FP, ONE, g[:2], g[:2] * 0, 8)
    with pytest.raises(ValueError, match='2 cascades for 3 rows'):
        _engine.curve_iir_dac_arguments(XP, FP, ONE[:2], g, g * 0, 8)
    with pytest.raises(ValueError, match='3 curves for 4 rows'):
        _engine.curve_iir_dac_arguments(XP, FP, ONE, g, g * 0, 8, batch=4)
    curve, dac, packed = _engine.curve_iir_dac_arguments(XP[0], FP[0], ONE, g, g * 0, 8, batch=3)    # one pair for every row
    assert curve[0].tolist() == [0, 3, 6, 9] and dac[0].tolist() == [1.0] * 3 and packed[1].shape == (3, 2)


@pytest.mark.parametrize('change,exc,message', BAD, ids=IDS)
def test_stage_refuses_before_any_device_work(change, exc, message):
    a = dict(OK, **change)
    if a['rows'] == [[]] * 3 and 'bits' not in change:
        message = 'a row without sections|sections is one'
    with pytest.raises(exc, match=message):
        distortion.CurveIirDacStage(a['xp'], a['fp'], a['rows'], a['n'], a['gain'], offset=a['offset'], bits=a['bits'],
                                    shift=a['shift'], left=a['left'], right=a['right'], dtype=a['dtype'])


def test_constructors_and_wrapper_refuse_before_any_device_work():
    with pytest.raises(NotImplementedError, match='CurveStage.*IirStage.*DacStage'):
        distortion.CurveIirDacStage(XP, FP, ONE, 8, 1000.0, interleave=2)
    for fs in (0.0, -1.0, np.inf, np.nan, [1.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match='full scale'):
            distortion.CurveIirDacStage.from_full_scale(XP, FP, ONE, 8, fs)
    with pytest.raises(ValueError, match='bits'):
        distortion.CurveIirDacStage.from_full_scale(XP, FP, ONE, 8, 1.0, bits=17)
    with pytest.raises(ValueError, match='2 gain entries for 3 rows'):
        distortion.CurveIirDacStage(XP, FP, ONE, 8, [1.0, 2.0])
    with pytest.raises(ValueError, match='4 cascades for 3 rows'):
        distortion.CurveIirDacStage(XP, FP, ONE + ONE[:1], 8, 1.0)
    with pytest.raises(ValueError, match='SOS matrix'):
        distortion.CurveIirDacStage(XP, FP, np.zeros((2, 5)), 8, 1.0)
    with pytest.raises(ValueError, match='2-D'):
        distortion.curve_iir_dac_rows(np.zeros(16), XP, FP, ONE, 1.0)
    with pytest.raises(NotImplementedError):
        distortion.curve_iir_dac_rows(np.zeros((3, 4)) + 0j, XP, FP, ONE, 1.0)
    with pytest.raises(ValueError, match='3 curves for 2 rows'):
        distortion.curve_iir_dac_rows(np.zeros((2, 4)), XP, FP, ONE, 1.0)
    with pytest.raises(ValueError, match='2 filter lists for 3 rows'):
        distortion.curve_iir_dac_rows(np.zeros((3, 4)), XP, FP, ONE[:2], 1.0)
    with pytest.raises(ValueError, match='row 0: gain is not finite'):
        distortion.curve_iir_dac_rows(np.zeros((3, 4)), XP, FP, ONE, [np.nan, 1.0, 1.0])
    with pytest.raises(ValueError, match='initial is a scalar or one value per row'):
        distortion.curve_iir_dac_rows(np.zeros((3, 4)), XP, FP, ONE, 1.0, initial=[0.0, 1.0])
    # nothing to look up: no device needed
    codes, counts, beyond = distortion.curve_iir_dac_rows(np.zeros((3, 0)), XP, FP, ONE, 1.0, return_counts=True)
    assert codes.shape == (3, 0) and codes.dtype == np.int16
    assert counts.shape == beyond.shape == (3, 3) and not counts.any() and not beyond.any()
    assert 'inverse_rows' in distortion.CurveIirDacStage.__doc__


def test_c_entry_refuses_before_any_device_work_curve_then_converter_then_cascade():
    lib = _engine.lib()
    orders = np.array([1], dtype=np.int32)
    b, a = np.array([[0.5, 0.25]] * 2), np.array([[1.0, -0.5]] * 2)
    g, o = np.array([1.0, 2.0]), np.array([0.0, 0.5])
    kp = np.array([0, 3, 5], dtype=np.int64)
    xp, fp = np.array([-1.0, 0.0, 2.0, 0.0, 1.0]), np.array([0.5, 0.0, 0.25, -1.0, 1.0])
    f64 = _engine._KIND_OF[np.dtype(np.float64)]
    h = C.c_void_p()
    ptr = lambda v: None if v is None else v.ctypes.data

    def create(n_sections=1, n=8, batch=2, kind=f64, knot_ptr=kp, xp=xp, fp=fp, gain=g, offset=o, bits=16, shift=0,
               orders=orders, a=a, out=C.byref(h)):
        return lib.wfk_curve_iir_dac_plan_create(n_sections, orders.ctypes.data, b.ctypes.data, a.ctypes.data, n, batch,
                                                 kind, ptr(knot_ptr), ptr(xp), ptr(fp), None, None, ptr(gain),
                                                 ptr(offset), bits, shift, out)

    bad_x = np.array([-1.0, 0.0, 2.0, 1.0, 1.0])
    bad_f = np.array([0.5, np.inf, 0.25, -1.0, 1.0])
    bad_a = np.array([[1.0, -0.5], [0.0, 1.0]])
    for kw, message in ((dict(out=None), b'null out'),
                        (dict(xp=None), b'bad curve rows plan arguments'),
                        (dict(batch=0), b'bad curve rows plan arguments'),
                        (dict(n=-1), b'bad curve rows plan arguments'),
                        (dict(kind=77), b'kind must be F64 or F32'),
                        (dict(knot_ptr=np.array([1, 3, 5], dtype=np.int64)), b'knot_ptr is not non-decreasing from 0'),
                        (dict(knot_ptr=np.array([0, 1, 5], dtype=np.int64)), b'row 0: fewer than 2 knots'),
                        (dict(xp=bad_x), b'row 1: knots are not strictly increasing at 1'),
                        (dict(fp=bad_f), b'row 0: value 1 is not finite'),
                        (dict(gain=None), b'bad dac rows plan arguments'),
                        (dict(bits=1), b'dac rows plan: bits must lie in [2, 16]'),
                        (dict(bits=14, shift=3), b'dac rows plan: shift must lie in [0, 16 - bits]'),
                        (dict(gain=np.array([1.0, np.nan])), b'row 1: gain is not finite'),
                        (dict(offset=np.array([np.inf, 0.0])), b'row 0: offset is not finite'),
                        (dict(n_sections=5, orders=np.array([1] * 5, dtype=np.int32)), b'state dimension <= 4'),
                        (dict(a=bad_a), b'a[0] must be finite and non-zero (row 1)'),
                        # a bad curve, a bad converter and a bad cascade: in that order
                        (dict(xp=bad_x, bits=1, a=bad_a), b'row 1: knots are not strictly increasing at 1'),
                        (dict(bits=1, a=bad_a), b'bits must lie in'),
                        (dict(gain=np.array([np.inf, 1.0]), n_sections=5, orders=np.array([1] * 5, dtype=np.int32)),
                         b'row 0: gain is not finite')):
        rc = create(**kw)
        assert rc < 0 and message in lib.wfk_last_error(), (kw, rc, lib.wfk_last_error())
        assert not h.value
    # the same texts as the curve's and the converter's own creators: one checker each
    d = C.c_void_p()
    assert lib.wfk_curve_rows_plan_create(8, 2, f64, kp.ctypes.data, bad_x.ctypes.data, fp.ctypes.data, None, None,
                                          C.byref(d)) < 0
    text = lib.wfk_last_error()
    assert create(xp=bad_x) < 0 and lib.wfk_last_error() == text
    assert lib.wfk_dac_rows_plan_create(8, 2, f64, g.ctypes.data, o.ctypes.data, 14, 3, 1, C.byref(d)) < 0
    text = lib.wfk_last_error()
    assert create(bits=14, shift=3) < 0 and lib.wfk_last_error() == text
    # NULL plans, as the siblings
    assert lib.wfk_curve_iir_dac_plan_destroy(None) == 0
    assert lib.wfk_curve_iir_dac_kernel_name(None) == b''
    assert lib.wfk_curve_iir_dac_state_dim(None) < 0
    assert lib.wfk_curve_iir_dac_apply(None, None, 0, None, 0, None, None, None, None, None, None) < 0
    assert b'null plan' in lib.wfk_last_error()
    assert lib.wfk_curve_iir_dac_apply_shared_in(None, None, None, 0, None, None, None, None, None, None) < 0
    assert b'null plan' in lib.wfk_last_error()


# ---- the sampler in front: SampledCurveIirDac -----------------------------------------------------------------------------
def _awg(rows=3, n=4096):
    import waveforms_amd as wf
    from waveforms_amd import workloads as wl
    return [wl.awg_channel(wf, c, n, 2e9) for c in range(rows)], wl.awg_grid(n, 2e9)


def test_sampled_plan_refuses_before_any_device_work():
    chans, grid = _awg()
    bad_xp = XP[:1] + [np.array([-1.0, -1.0, 2.0])] + XP[:1]
    for kw, exc, message in ((dict(xp=bad_xp), ValueError, 'row 1: knots are not strictly increasing at 1'),
                             (dict(xp=XP[:2], fp=FP[:2]), ValueError, '2 curves for 3 rows'),
                             (dict(fp=FP[:2] + [np.array([0.0, np.nan, 1.0])]), ValueError, 'row 2: value 1 is not finite'),
                             (dict(left=[0.0, 1.0]), ValueError, '2 values of left for 3 rows'),
                             (dict(bits=17), ValueError, r'bits must lie in \[2, 16\]'),
                             (dict(bits=14, shift=3), ValueError, r'shift must lie in \[0, 16 - bits\]'),
                             (dict(gain=[1.0, np.nan, 1.0]), ValueError, 'row 1: gain is not finite'),
                             (dict(gain=[1.0, 2.0]), ValueError, '2 gain entries for 3 rows'),
                             (dict(rows=ONE[:2]), ValueError, '2 cascades for 3 rows'),
                             (dict(rows=[[([1.0] * 6, [1.0, -0.1, 0.0, 0.0, 0.0, 0.01])]] * 3), NotImplementedError,
                              'state dimension <= 4'),
                             # the curve's first, then the converter's, then the cascade's
                             (dict(xp=bad_xp, bits=17, rows=ONE[:2]), ValueError, 'row 1: knots are not strictly'),
                             (dict(bits=17, rows=ONE[:2]), ValueError, r'bits must lie in \[2, 16\]')):
        a = dict(dict(xp=XP, fp=FP, rows=ONE, gain=1000.0, offset=0.0, bits=16, shift=0, left=None), **kw)
        with pytest.raises(exc, match=message):
            distortion.SampledCurveIirDac(chans, grid, a['xp'], a['fp'], a['rows'], a['gain'], offset=a['offset'],
                                          bits=a['bits'], shift=a['shift'], left=a['left'])
    with pytest.raises(NotImplementedError, match='complex'):
        distortion.SampledCurveIirDac([c * (1 + 0.5j) for c in chans], grid, XP, FP, ONE, 1000.0)
    for fs in (0.0, np.nan, [1.0, -1.0, 1.0]):
        with pytest.raises(ValueError, match='full scale'):
            distortion.SampledCurveIirDac.from_full_scale(chans, grid, XP, FP, ONE, fs)
    assert 'inverse_rows' in distortion.SampledCurveIirDac.__doc__


def test_chain_c_entry_refuses_before_any_device_work_curve_then_converter_then_cascade():
    from waveforms_amd import _flatten
    chans, grid_desc = _awg(2)
    grid = grid_desc if isinstance(grid_desc, _flatten.wfk_grid) else _flatten.grid_from_desc(grid_desc)
    prog = _flatten.flatten(chans, grid, None)
    lib = _engine.lib()
    orders = np.array([1], dtype=np.int32)
    b, a = np.array([[0.5, 0.25]] * 2), np.array([[1.0, -0.5]] * 2)
    g, o = np.array([1.0, 2.0]), np.array([0.0, 0.5])
    kp = np.array([0, 3, 5], dtype=np.int64)
    xp, fp = np.array([-1.0, 0.0, 2.0, 0.0, 1.0]), np.array([0.5, 0.0, 0.25, -1.0, 1.0])
    h = C.c_void_p()
    ptr = lambda v: None if v is None else v.ctypes.data

    def create(n_sections=1, knot_ptr=kp, xp=xp, fp=fp, gain=g, offset=o, bits=16, shift=0, orders=orders, a=a,
               prog=C.byref(prog.struct), out=C.byref(h)):
        return lib.wfk_chain_curve_iir_dac_plan_create(prog, C.byref(grid), n_sections, orders.ctypes.data,
                                                       b.ctypes.data, a.ctypes.data, ptr(knot_ptr), ptr(xp), ptr(fp),
                                                       None, None, ptr(gain), ptr(offset), bits, shift, out)

    bad_x = np.array([-1.0, 0.0, 2.0, 1.0, 1.0])
    bad_a = np.array([[1.0, -0.5], [0.0, 1.0]])
    for kw, message in ((dict(out=None), b'null out'),
                        (dict(prog=None), b'null argument'),
                        (dict(fp=None), b'bad curve rows plan arguments'),
                        (dict(knot_ptr=np.array([0, 1, 5], dtype=np.int64)), b'row 0: fewer than 2 knots'),
                        (dict(xp=bad_x), b'row 1: knots are not strictly increasing at 1'),
                        (dict(gain=None), b'bad dac rows plan arguments'),
                        (dict(bits=1), b'dac rows plan: bits must lie in [2, 16]'),
                        (dict(offset=np.array([np.inf, 0.0])), b'row 0: offset is not finite'),
                        (dict(n_sections=5, orders=np.array([1] * 5, dtype=np.int32)), b'state dimension <= 4'),
                        (dict(a=bad_a), b'a[0] must be finite and non-zero (row 1)'),
                        (dict(xp=bad_x, bits=1, a=bad_a), b'row 1: knots are not strictly increasing at 1'),
                        (dict(bits=1, a=bad_a), b'bits must lie in')):
        rc = create(**kw)
        assert rc < 0 and message in lib.wfk_last_error(), (kw, rc, lib.wfk_last_error())
        assert not h.value
    # NULL plans, as the siblings
    assert lib.wfk_chain_curve_iir_dac_plan_destroy(None) == 0
    assert lib.wfk_chain_curve_iir_dac_kernel_name(None) == b''
    assert lib.wfk_chain_curve_iir_dac_unfused_reason(None) == b''
    assert lib.wfk_chain_curve_iir_dac_is_fused(None) == 0 and lib.wfk_chain_curve_iir_dac_state_dim(None) < 0
    assert lib.wfk_chain_curve_iir_dac_table_bytes(None) < 0
    assert lib.wfk_chain_curve_iir_dac_launch(None, None, 0, None, None, None, 0, None, None, None, None) < 0
    assert b'null plan' in lib.wfk_last_error()
