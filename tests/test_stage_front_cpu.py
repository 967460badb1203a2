"""The shared Python front of the stages that end in int16 DAC codes (the private helpers of
waveforms_amd/distortion.py; DESIGN.md, "The row rule"): the full-scale gain, the per-row converter arguments, cascades
spelt three ways, the one order of the tensor refusals, and `initial` on the host.  Metadata and integers only: the
tensors are stand-ins that hold nothing but what the checks read.  No device, no library load."""
import re

import numpy as np
import pytest
import torch

from waveforms_amd import _rows
from waveforms_amd import distortion as d

WHO = 'SomeStage'


# ------------------------------------------------------------------ full-scale gain
@pytest.mark.parametrize('bits', [2, 14, 16])
def test_full_scale_gain(bits):
    fs = np.array([0.5, 1.0, 3.0])
    hi = 2**(bits - 1) - 1
    assert np.array_equal(d._full_scale_gain(WHO, fs, {'bits': bits, 'shift': 1}), hi / fs)
    assert d._full_scale_gain(WHO, 2.0, {'bits': bits}) == hi / 2.0              # a scalar stays one


def test_full_scale_gain_defaults_to_16_bits():
    assert d._full_scale_gain(WHO, 1.0, {}) == 32767.0


@pytest.mark.parametrize('bad', [0.0, -1.0, np.inf, np.nan, [1.0, 0.0], [1.0, np.nan]])
def test_full_scale_refused(bad):
    with pytest.raises(ValueError, match=f'^{WHO}: every full scale must be finite and positive$'):
        d._full_scale_gain(WHO, bad, {})


@pytest.mark.parametrize('bits', [1, 17])
def test_full_scale_bits_refused(bits):
    with pytest.raises(ValueError, match=re.escape('bits must lie in [2, 16]')):
        d._full_scale_gain(WHO, 1.0, {'bits': bits})
    with pytest.raises(ValueError, match=re.escape('bits must lie in [2, 16]')):          # before the full scale
        d._full_scale_gain(WHO, -1.0, {'bits': bits})


# ------------------------------------------------------------------ per-row converter arguments
@pytest.mark.parametrize('value,want', [
    (2.5, [2.5] * 3), (np.float64(2.5), [2.5] * 3), (np.array(2.5), [2.5] * 3),
    ([1.0, 2.0, 3.0], [1.0, 2.0, 3.0]), (np.array([1.0, 2.0, 3.0]), [1.0, 2.0, 3.0]),
    (np.array([[1.0], [2.0], [3.0]]), [1.0, 2.0, 3.0])])
def test_per_row_arguments(value, want):
    gains, offsets = d._gain_offset_rows(WHO, value, 0.0, 3)
    assert isinstance(gains, list) and [float(g) for g in gains] == want and offsets == [0.0] * 3
    gains, offsets = d._gain_offset_rows(WHO, 1.0, value, 3)
    assert isinstance(offsets, list) and [float(o) for o in offsets] == want and gains == [1.0] * 3


def test_per_row_arguments_refused():
    with pytest.raises(ValueError, match=f'^{WHO}: 2 gain entries for 3 rows$'):
        d._gain_offset_rows(WHO, [1.0, 2.0], 0.0, 3)
    with pytest.raises(ValueError, match=f'^{WHO}: 4 offset entries for 3 rows$'):
        d._gain_offset_rows(WHO, 1.0, np.zeros(4), 3)
    with pytest.raises(ValueError, match=f'^{WHO}: 2 gain entries for 3 rows$'):           # the gain first
        d._gain_offset_rows(WHO, [1.0, 2.0], np.zeros(4), 3)
    with pytest.raises(ValueError, match=f'^{WHO}: 2 lead entries for 3 rows$'):
        d._per_row_flat(WHO, 'lead', np.array([4, 5]), 3)


# ------------------------------------------------------------------ cascades to rows
SPELLING = 'spelt as the stage spells it'
ONE = [([1.0, 0.5], [1.0, -0.25]), ([0.5, 0.0], [1.0, -0.5])]


def test_cascades_from_an_sos_matrix():
    sos = np.array([[1.0, 0.5, 0.0, 1.0, -0.25, 0.0], [0.5, 0.0, 0.0, 1.0, -0.5, 0.0]])
    for matrix in (sos, sos.tolist()):
        rows, one = d._cascade_rows(WHO, matrix, 3, SPELLING)
        assert len(rows) == 3 and all(len(r) == 2 for r in rows) and len(one) == 2
        for r in rows:
            for (b, a), (b1, a1), line in zip(r, one, sos):
                assert np.array_equal(b, line[:3]) and np.array_equal(a, line[3:])
                assert b is b1 and a is a1


def test_one_cascade_goes_to_every_row():
    rows, one = d._cascade_rows(WHO, ONE, 2, SPELLING)
    assert one is ONE and rows == [ONE, ONE]
    rows, one = d._cascade_rows(WHO, ONE, None, SPELLING, one_for=4)                # the rows are not given: `one_for`
    assert one is ONE and rows == [ONE] * 4
    arrays = [(np.array(b), np.array(a)) for b, a in ONE]                          # coefficient arrays nest alike
    assert d._cascade_rows(WHO, arrays, 1, SPELLING)[1] is arrays


def test_one_cascade_per_row():
    per_row = [ONE, ONE[:1], ONE[1:]]
    for rows_given in (3, None):                                                   # None: the cascades decide
        rows, one = d._cascade_rows(WHO, per_row, rows_given, SPELLING, one_for=7)
        assert one is None and rows == per_row
    assert d._cascade_rows(WHO, tuple(per_row), 3, SPELLING)[0] == per_row         # a list comes back


def test_cascades_refused():
    with pytest.raises(ValueError, match=f'^{WHO}: 2 cascades for 3 rows$'):
        d._cascade_rows(WHO, [ONE, ONE], 3, SPELLING)
    with pytest.raises(ValueError, match=f'^{WHO}: 0 cascades for 0 rows$'):
        d._cascade_rows(WHO, ONE, 0, SPELLING)
    with pytest.raises(ValueError, match=re.escape(f'{WHO}: an SOS matrix has shape (n_sections, 6)')):
        d._cascade_rows(WHO, np.ones((2, 5)), 3, SPELLING)
    for sections in ([1.0, 0.5], 1.0, [], [[ONE]]):                                # depths 1, 0, 0 and 5
        with pytest.raises(ValueError, match=f'^{WHO}: sections is {SPELLING}$'):
            d._cascade_rows(WHO, sections, 3, SPELLING)


# ------------------------------------------------------------------ codes, reports and state
class Meta:
    """what the checks may read of a tensor, and nothing else: anything further is an AttributeError"""

    def __init__(self, ptr, shape, strides, dtype, is_cuda=True, contiguous=True):
        self.is_cuda, self.dtype, self.shape = is_cuda, dtype, tuple(shape)
        self._ptr, self._strides, self._contiguous = ptr, tuple(strides), contiguous

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self._strides[i]

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return self._contiguous


ROWS, N, SD = 2, 8, 2
X0, Y0, C0, ZI, ZF = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
X_BYTES, Y_BYTES, REPORT_BYTES = ROWS * N * 8, ROWS * N * 2, ROWS * 24
REFUSALS = [
    'expected x: (batch, >=n) row-contiguous device tensor of the stage dtype, or one row',
    'expected codes: (batch, >=n) row-contiguous int16 device tensor',
    'expected counts: contiguous (batch, 3) int64 device tensor',
    'expected beyond: contiguous (batch, 3) int64 device tensor',
    'zi / zf must be contiguous (batch, state_dim) float64 device tensors',
    'curve iir dac stage is out of place: codes overlaps x',
    'curve iir dac stage: counts overlaps x / codes',
    'curve iir dac stage: beyond overlaps x / codes',
    'curve iir dac stage: beyond overlaps counts',
]


def report(at):
    return Meta(at, (ROWS, 3), (3, 1), torch.int64)


def tensors(passed):
    """the arguments with the first `passed` conditions of REFUSALS met and EVERY later one broken, each overlap the
    smallest there is: x ends on the first byte of codes, a report begins on the last byte of codes, beyond begins
    8 bytes before the end of counts"""
    x = Meta(X0 if passed > 5 else Y0 - X_BYTES + 1, (ROWS, N), (N, 1), torch.float64 if passed > 0 else torch.float32)
    codes = Meta(Y0, (ROWS, N), (N, 1), torch.int16 if passed > 1 else torch.int32)
    counts = Meta(C0 if passed > 6 else Y0 + Y_BYTES - 1, (ROWS, 3), (3, 1), torch.int64, contiguous=passed > 2)
    at = C0 + REPORT_BYTES if passed > 8 else C0 + REPORT_BYTES - 8 if passed > 7 else Y0 + Y_BYTES - 1
    beyond = Meta(at, (ROWS, 3) if passed > 3 else (ROWS, 2), (3, 1), torch.int64)
    zi = Meta(ZI, (ROWS, SD), (SD, 1), torch.float64)
    zf = Meta(ZF, (ROWS, SD), (SD, 1), torch.float64 if passed > 4 else torch.float32)
    return x, codes, counts, beyond, zi, zf


@pytest.mark.parametrize('passed', range(len(REFUSALS)))
def test_refusals_come_in_one_order(passed):
    """through a stage's own `apply_torch` (its two row checks, then the shared one), on a stage without a plan: every
    refusal comes before the plan is looked at"""
    stage = object.__new__(d.CurveIirDacStage)
    stage.batch, stage.n, stage.dtype, stage.state_dim = ROWS, N, np.dtype(np.float64), SD
    x, codes, counts, beyond, zi, zf = tensors(passed)
    with pytest.raises(ValueError, match=f'^{re.escape(REFUSALS[passed])}$'):
        stage.apply_torch(x, codes, counts=counts, beyond=beyond, zi=zi, zf=zf)


def sides_of(x, codes, x_rows=ROWS):
    """as a stage builds them: the pointers and strides that check_rows gives"""
    x0, xs = _rows.check_rows(x, x_rows, N, torch.float64, '')
    y0, ys = _rows.check_rows(codes, ROWS, N, torch.int16, '')
    return (x0, xs, x_rows, N, 8), (y0, ys, ROWS, N, 2)


def check(sides, counts=None, beyond=None, zi=None, zf=None):
    return d._check_reports('the stage', 'codes', 'batch', ROWS, sides, counts, beyond, zi, zf, SD)


def test_accepted_tensors_give_their_pointers():
    x, codes, counts, beyond, zi, zf = tensors(len(REFUSALS))
    assert check(sides_of(x, codes), counts, beyond, zi, zf) == (C0, C0 + REPORT_BYTES, ZI, ZF)
    assert check(sides_of(x, codes)) == (None, None, None, None)
    assert check(sides_of(x, codes), None, beyond, None, zf) == (None, C0 + REPORT_BYTES, None, ZF)
    # what touches without meeting: x ends where codes begin, the reports follow codes and each other
    x = Meta(Y0 - X_BYTES, (ROWS, N), (N, 1), torch.float64)
    got = check(sides_of(x, codes), report(Y0 + Y_BYTES), report(Y0 + Y_BYTES + REPORT_BYTES))
    assert got == (Y0 + Y_BYTES, Y0 + Y_BYTES + REPORT_BYTES, None, None)
    # beyond in FRONT of counts, its last 8 bytes on them
    with pytest.raises(ValueError, match='^the stage: beyond overlaps counts$'):
        check(sides_of(x, codes), report(C0), report(C0 - REPORT_BYTES + 8))
    assert check(sides_of(x, codes), report(C0), report(C0 - REPORT_BYTES))[:2] == (C0, C0 - REPORT_BYTES)


def test_one_row_of_x_below_its_stride():
    """ONE input row that every row reads (the shared-input form): torch may give a (1, n) view any stride(0), so n
    stands in for it, in what is passed down and in the bytes the row occupies"""
    codes = Meta(Y0, (ROWS, N), (N, 1), torch.int16)

    def shared(x0):
        sides = sides_of(Meta(x0, (1, N), (1, 1), torch.float64), codes, x_rows=1)
        assert sides[0][:2] == (x0, N)
        return check(sides, report(C0))
    assert shared(Y0 - N * 8) == shared(Y0 + Y_BYTES) == (C0, None, None, None)
    for x0 in (Y0 - N * 8 + 1, Y0 + Y_BYTES - 1):
        with pytest.raises(ValueError, match='^the stage is out of place: codes overlaps x$'):
            shared(x0)
    with pytest.raises(ValueError, match='^the stage: counts overlaps x / codes$'):
        shared(C0 - N * 8 + 1)


def test_a_sampled_chain_has_no_input():
    side = (Y0, N + 2, ROWS, N, 2)                                   # code rows that are a window of a wider tensor
    last = Y0 + ((ROWS - 1) * (N + 2) + N) * 2 - 1                  # the last byte of the last row, not of the buffer

    def chain(counts, beyond=None):
        return d._check_reports('the chain', 'codes', 'n_channels', ROWS, (side, ), counts, beyond)
    assert chain(report(C0), report(C0 + REPORT_BYTES)) == (C0, C0 + REPORT_BYTES, None, None)
    assert chain(None, report(C0)) == (None, C0, None, None)
    assert chain(report(last + 1)) == (last + 1, None, None, None)
    with pytest.raises(ValueError, match=re.escape('expected counts: contiguous (n_channels, 3) int64 device tensor')):
        chain(Meta(C0, (ROWS, 3), (3, 1), torch.int32))
    with pytest.raises(ValueError, match=re.escape('expected beyond: contiguous (n_channels, 3) int64 device tensor')):
        chain(report(C0), Meta(C0 + REPORT_BYTES, (ROWS, 3), (3, 1), torch.int64, is_cuda=False))
    with pytest.raises(ValueError, match='^the chain: counts overlaps codes$'):
        chain(report(last))
    with pytest.raises(ValueError, match='^the chain: beyond overlaps codes$'):
        chain(report(C0), report(last))
    with pytest.raises(ValueError, match='^the chain: beyond overlaps counts$'):
        chain(report(C0), report(C0 + REPORT_BYTES - 8))


def test_state_pointers():
    zi, zf = Meta(ZI, (ROWS, SD), (SD, 1), torch.float64), Meta(ZF, (ROWS, SD), (SD, 1), torch.float64)
    assert d._state_ptrs(None, None, ROWS, SD, 'batch') == (None, None)
    assert d._state_ptrs(zi, None, ROWS, SD, 'batch') == (ZI, None)
    assert d._state_ptrs(zi, zf, ROWS, SD, 'batch') == (ZI, ZF)
    text = re.escape('zi / zf must be contiguous (n_channels, state_dim) float64 device tensors')
    for bad in (Meta(ZF, (ROWS, SD + 1), (SD + 1, 1), torch.float64), Meta(ZF, (ROWS, SD), (SD, 1), torch.float32),
                Meta(ZF, (ROWS, SD), (SD, 1), torch.float64, contiguous=False),
                Meta(ZF, (ROWS, SD), (SD, 1), torch.float64, is_cuda=False)):
        for pair in ((bad, None), (None, bad), (zi, bad)):
            with pytest.raises(ValueError, match=f'^{text}$'):
                d._state_ptrs(*pair, ROWS, SD, 'n_channels')


# ------------------------------------------------------------------ `initial` on the host
def test_host_initial():
    text = 'some_rows: initial is a scalar or one value per row'
    for scalar in (0.25, np.float32(0.25), np.array(0.25), 1):
        got = d._initial_host(scalar, 3, text)
        assert got.dtype == np.float64 and got.shape == (3, ) and np.all(got == float(scalar))
    got = d._initial_host([1, 2, 3], 3, text)
    assert got.dtype == np.float64 and np.array_equal(got, [1.0, 2.0, 3.0])
    for bad in (np.zeros((3, 1)), np.zeros((1, 3)), [1.0, 2.0], np.zeros(4), []):
        with pytest.raises(ValueError, match=f'^{text}$'):
            d._initial_host(bad, 3, text)
