"""The per-row IIR stage that ends in DAC codes (distortion.IirDacStage / iir_dac_rows, csrc/wfk_iir_rows_dac.hip)
without a device: every refusal before any device work (the stage, the plan, the C entry through ctypes), the symbols
and what they return for a NULL plan, the referee (tests/iir_dac_ref.py) against hand-worked rows, and the condition
the GPU test's comparison with the referee rests on: the undecided share of each of its inputs, computed from the
referee alone."""
import ctypes as C

import numpy as np
import pytest

import dac_rows_ref
import iir_dac_ref as ref
from waveforms_amd import _engine, distortion

ONE = [[([0.5, 0.25], [1.0, -0.5])]] * 3        # three rows, one first-order section each


# ---- refusals ---------------------------------------------------------------------------------------------------------
OK = dict(n=8, gain=1000.0, offset=0.0, bits=16, shift=0, dtype=np.float64)
BAD = [   # (cascades, what differs from OK, exception, message)
    (ONE, dict(bits=1), ValueError, r'bits must lie in \[2, 16\]'),
    (ONE, dict(bits=17), ValueError, r'bits must lie in \[2, 16\]'),
    (ONE, dict(bits=16, shift=1), ValueError, r'shift must lie in \[0, 16 - bits\]'),
    (ONE, dict(bits=12, shift=-1), ValueError, r'shift must lie in \[0, 16 - bits\]'),
    (ONE, dict(n=-1), ValueError, 'n >= 0'),
    (ONE, dict(gain=[1.0, np.inf, 1.0]), ValueError, 'row 1: gain is not finite'),
    (ONE, dict(offset=[0.0, 0.0, np.nan]), ValueError, 'row 2: offset is not finite'),
    (ONE, dict(gain=[1.0, 2.0]), ValueError, '2 gain entries for 3 rows'),
    (ONE, dict(offset=[0.0] * 4), ValueError, '4 offset entries for 3 rows'),
    (ONE, dict(dtype=np.int16), ValueError, 'dtype must be float64 or float32'),
    (ONE, dict(dtype=np.complex128), NotImplementedError, 'complex'),
    ([[([1.0, 0.5j], [1.0, -0.5])]], {}, NotImplementedError, 'complex coefficients'),
    ([[]], {}, ValueError, 'sections is one'),
    ([[([1.0] * 6, [1.0, -0.1, 0.0, 0.0, 0.0, 0.01])]] * 2, {}, NotImplementedError, 'state dimension <= 4'),
    ([[([1.0, 0.1, 0.1], [1.0, -0.1, 0.1])] * 3] * 2, {}, NotImplementedError, 'state dimension <= 4'),
    ([[([1.0, 0.1], [0.0, 1.0])]] * 2, {}, _engine.EngineError, r'a\[0\] must be finite and non-zero'),
]


@pytest.mark.parametrize('rows,change,exc,message', BAD, ids=[f'{i}-{b[3][:24]}' for i, b in enumerate(BAD)])
def test_stage_refuses_before_any_device_work(rows, change, exc, message):
    a = dict(OK, **change)
    with pytest.raises(exc, match=message):
        distortion.IirDacStage(rows, a['n'], a['gain'], offset=a['offset'], bits=a['bits'], shift=a['shift'],
                               dtype=a['dtype'])


def test_interleave_is_refused_with_the_route():
    with pytest.raises(NotImplementedError, match='IirStage.*DacStage'):
        distortion.IirDacStage(ONE, 8, 1000.0, interleave=2)


def test_constructors_and_wrapper_refuse_before_any_device_work():
    for fs in (0.0, -1.0, np.inf, np.nan, [1.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match='full scale'):
            distortion.IirDacStage.from_full_scale(ONE, 8, fs)
    with pytest.raises(ValueError, match='bits'):
        distortion.IirDacStage.from_full_scale(ONE, 8, 1.0, bits=17)
    with pytest.raises(ValueError, match='4 cascades for 3 rows'):
        distortion.IirDacStage(ONE + ONE[:1], 8, 1.0, batch=3)
    with pytest.raises(ValueError, match='SOS matrix'):
        distortion.IirDacStage(np.zeros((2, 5)), 8, [1.0, 1.0])
    with pytest.raises(ValueError, match='2-D'):
        distortion.iir_dac_rows(np.zeros(16), ONE, 1.0)
    with pytest.raises(NotImplementedError):
        distortion.iir_dac_rows(np.zeros((3, 4)) + 0j, ONE, 1.0)
    with pytest.raises(ValueError, match='3 filter lists for 2 rows'):
        distortion.iir_dac_rows(np.zeros((2, 4)), ONE, 1.0)
    with pytest.raises(ValueError, match='row 0: gain is not finite'):
        distortion.iir_dac_rows(np.zeros((3, 4)), ONE, [np.nan, 1.0, 1.0])
    with pytest.raises(ValueError, match='initial is a scalar or one value per row'):
        distortion.iir_dac_rows(np.zeros((3, 4)), ONE, 1.0, initial=[0.0, 1.0])
    # nothing to filter: no device needed
    codes, counts = distortion.iir_dac_rows(np.zeros((3, 0)), ONE, 1.0, return_counts=True)
    assert codes.shape == (3, 0) and codes.dtype == np.int16 and counts.shape == (3, 3) and not counts.any()


def test_c_entry_refuses_before_any_device_work_with_the_converters_texts():
    lib = _engine.lib()
    orders = np.array([1], dtype=np.int32)
    b, a = np.array([[0.5, 0.25]] * 2), np.array([[1.0, -0.5]] * 2)
    g, o = np.array([1.0, 2.0]), np.array([0.0, 0.5])
    h = C.c_void_p()

    def create(n_sections=1, n=8, batch=2, kind=_engine._KIND_OF[np.dtype(np.float64)], gain=g, offset=o, bits=16, shift=0,
               orders=orders, out=C.byref(h)):
        return lib.wfk_iir_rows_dac_plan_create(n_sections, orders.ctypes.data, b.ctypes.data, a.ctypes.data, n, batch,
                                                kind, None if gain is None else gain.ctypes.data,
                                                None if offset is None else offset.ctypes.data, bits, shift, out)

    for kw, message in ((dict(out=None), b'null out'),
                        (dict(gain=None), b'bad dac rows plan arguments'),
                        (dict(batch=0), b'bad dac rows plan arguments'),
                        (dict(bits=1), b'dac rows plan: bits must lie in [2, 16]'),
                        (dict(bits=14, shift=3), b'dac rows plan: shift must lie in [0, 16 - bits]'),
                        (dict(gain=np.array([1.0, np.nan])), b'row 1: gain is not finite'),
                        (dict(offset=np.array([np.inf, 0.0])), b'row 0: offset is not finite'),
                        (dict(n=-1), b'bad per-row IIR arguments'),
                        (dict(kind=77), b'IIR kind must be F64 or F32'),
                        (dict(n_sections=5, orders=np.array([1] * 5, dtype=np.int32)), b'state dimension <= 4'),
                        # the converter's refusal comes first
                        (dict(bits=1, n=-1), b'bits must lie in')):
        rc = create(**kw)
        assert rc < 0 and message in lib.wfk_last_error(), (kw, rc, lib.wfk_last_error())
        assert not h.value
    # the same texts as the converter's own creator: one checker
    d = C.c_void_p()
    assert lib.wfk_dac_rows_plan_create(8, 2, _engine._KIND_OF[np.dtype(np.float64)], g.ctypes.data, o.ctypes.data, 14,
                                        3, 1, C.byref(d)) < 0
    text = lib.wfk_last_error()
    assert create(bits=14, shift=3) < 0 and lib.wfk_last_error() == text
    # NULL plans
    assert lib.wfk_iir_rows_dac_plan_destroy(None) == 0
    assert lib.wfk_iir_rows_dac_kernel_name(None) == b''
    assert lib.wfk_iir_rows_dac_state_dim(None) < 0
    assert lib.wfk_iir_rows_dac_apply(None, None, 0, None, 0, None, None, None, None, None) < 0
    assert b'null plan' in lib.wfk_last_error()
    assert lib.wfk_iir_rows_dac_apply_shared_in(None, None, None, 0, None, None, None, None, None) < 0


def test_sampled_plan_refuses_before_any_device_work():
    import waveforms_amd as wf
    from waveforms_amd import workloads as wl
    chans = [wl.awg_channel(wf, c, 4096, 2e9) for c in range(3)]
    grid = wl.awg_grid(4096, 2e9)
    for kw, exc, message in ((dict(bits=17), ValueError, r'bits must lie in \[2, 16\]'),
                             (dict(bits=14, shift=3), ValueError, r'shift must lie in \[0, 16 - bits\]'),
                             (dict(gain=[1.0, np.nan, 1.0]), ValueError, 'row 1: gain is not finite'),
                             (dict(gain=[1.0, 2.0]), ValueError, '2 gain entries for 3 rows'),
                             (dict(offset=[0.0] * 4), ValueError, '4 offset entries for 3 rows'),
                             (dict(rows=ONE[:2]), ValueError, '2 cascades for 3 rows'),
                             (dict(rows=[[([1.0] * 6, [1.0, -0.1, 0.0, 0.0, 0.0, 0.01])]] * 3), NotImplementedError,
                              'state dimension <= 4')):
        a = dict(dict(rows=ONE, gain=1000.0, offset=0.0, bits=16, shift=0), **kw)
        with pytest.raises(exc, match=message):
            distortion.SampledIirDac(chans, grid, a['rows'], a['gain'], offset=a['offset'], bits=a['bits'], shift=a['shift'])
    with pytest.raises(NotImplementedError, match='complex'):
        distortion.SampledIirDac([c * (1 + 0.5j) for c in chans], grid, ONE, 1000.0)
    for fs in (0.0, np.nan, [1.0, -1.0, 1.0]):
        with pytest.raises(ValueError, match='full scale'):
            distortion.SampledIirDac.from_full_scale(chans, grid, ONE, fs)
    lib = _engine.lib()
    assert lib.wfk_chain_iir_rows_dac_plan_destroy(None) == 0
    assert lib.wfk_chain_iir_rows_dac_kernel_name(None) == b'' and lib.wfk_chain_iir_rows_dac_unfused_reason(None) == b''
    assert lib.wfk_chain_iir_rows_dac_is_fused(None) == 0 and lib.wfk_chain_iir_rows_dac_state_dim(None) < 0
    assert lib.wfk_chain_iir_rows_dac_launch(None, None, 0, None, None, 0, None, None, None, None) < 0


# ---- the referee against hand-worked rows -----------------------------------------------------------------------------
def test_referee_on_hand_worked_rows():
    # y[i] = 0.5 x[i] + 0.25 x[i-1] + 0.5 y[i-1] from a zero state: x = 4, 0, 0, 8 -> y = 2, 2, 1, 4.5
    secs = [([0.5, 0.25], [1.0, -0.5])]
    y, zf = ref.cascade(secs, [4.0, 0.0, 0.0, 8.0], np.zeros(1))
    assert y.tolist() == [2.0, 2.0, 1.0, 4.5] and zf.tolist() == [0.25 * 8.0 + 0.5 * 4.5]
    # around a level: the level passes unchanged where the filter has unit DC gain (0.75 / 0.5 = 1.5 here: it does not)
    y1, _ = ref.cascade(secs, [1.0, 1.0], np.zeros(1), initial=1.0)
    assert y1.tolist() == [1.0, 1.0]
    # ties go to even: y * 0.5 + 0.5 = 1.5, 1.5, 1.0, 2.75 -> 2, 2, 1, 3;  * 0.25 + 0 = 0.5, 0.5, 0.25, 1.125 -> 0, 0, 0, 1
    row = y[None, :]
    codes, counts = dac_rows_ref.dac_ref(row, 0.5, 0.5)
    assert codes.tolist() == [[2, 2, 1, 3]] and counts.tolist() == [[0, 0, 0]]
    codes, _ = dac_rows_ref.dac_ref(row, 0.25, 0.0)
    assert codes.tolist() == [[0, 0, 0, 1]]
    codes, _ = dac_rows_ref.dac_ref(row, -1.25, 0.0)                   # -2.5, -2.5, -1.25, -5.625 -> -2, -2, -1, -6
    assert codes.tolist() == [[-2, -2, -1, -6]]
    # both rails, 3 bits (lo = -4, hi = 3), shift 2: v = 2 y - 4 = 0, 0, -2, 5 -> 0, 0, -2, 3 (above) -> * 4
    codes, counts = dac_rows_ref.dac_ref(row, 2.0, -4.0, bits=3, shift=2)
    assert codes.tolist() == [[0, 0, -8, 12]] and counts.tolist() == [[0, 1, 0]]
    codes, counts = dac_rows_ref.dac_ref(row, -2.0, 0.0, bits=3, shift=13)   # -4, -4, -2, -9 -> -4, -4, -2, -4 (below)
    assert codes.tolist() == [[-32768, -32768, -16384, -32768]] and counts.tolist() == [[1, 0, 0]]
    # v = hi + 0.5 = 3.5 rounds to 4 > hi: above; v = 2.5 -> 2; v = lo - 0.5 = -4.5 -> -4: not below
    codes, counts = dac_rows_ref.dac_ref(np.array([[3.5, 2.5, -4.5]]), 1.0, 0.0, bits=3)
    assert codes.tolist() == [[3, 2, -4]] and counts.tolist() == [[0, 1, 0]]
    # a NaN in mid-row stays in the state: every code from it on is 0 and counted
    yn, _ = ref.cascade(secs, [4.0, np.nan, 0.0, 8.0], np.zeros(1))
    codes, counts = dac_rows_ref.dac_ref(yn[None, :], 1.0, 0.25)
    assert codes.tolist() == [[2, 0, 0, 0]] and counts.tolist() == [[0, 0, 3]]


def test_case_gains_clip_on_both_rails_with_both_signs():
    for bits, shift in ref.FORMATS:
        case = ref.Case(1, 3, 3, ref.TILE + 1, bits, shift)
        codes, counts = case.reference()
        assert (case.gain[::2] > 0).all() and (case.gain[1::2] < 0).all()
        assert (counts[:, 0] > 0).all() and (counts[:, 1] > 0).all() and not counts[:, 2].any()
        assert np.all(case.offset != np.round(case.offset))
        assert (counts[:, :2].sum(axis=1) < case.n // 2).all()          # most samples are inside the rails


# ---- the decided-samples condition, from the referee alone ------------------------------------------------------------
def test_undecided_share_of_the_gpu_tests_inputs():
    for case in ref.referee_cases():
        tol = case.tol_y()
        mask, near_lo, near_hi = case.undecided(tol)
        share = mask.mean(axis=1)
        delta = np.abs(case.gain) * tol
        print(f'shape ({case.nsec}, {case.order}) n {case.n} bits {case.bits}: tol_y {tol.max():.3g}, delta '
              f'{delta.max():.3g} LSB, undecided {int(mask.sum())} (share {share.max():.3g}), at the rails '
              f'{int(near_lo.sum())} / {int(near_hi.sum())}')
        assert (share <= ref.MAX_UNDECIDED_SHARE).all(), (case.nsec, case.order, case.n, case.bits, share)


def test_undecided_marks_what_it_should():
    case = ref.Case(1, 1, 1, 64)
    case.gain, case.offset = np.array([1.0]), np.array([0.0])
    case.y = np.array([[0.5, 0.5 + 1e-6, 0.25, -32768.5, 32767.5 - 1e-7, 7.0]])
    mask, near_lo, near_hi = case.undecided(np.array([1e-6]))
    assert mask.tolist() == [[True, True, False, True, True, False]]
    assert near_lo.tolist() == [[False, False, False, True, False, False]]
    assert near_hi.tolist() == [[False, False, False, False, True, False]]
