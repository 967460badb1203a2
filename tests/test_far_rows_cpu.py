"""The geometry of `row_windows.FarWindow` as arithmetic on Python integers, and the row rule's Python side at a far
stride.  Nothing is allocated and no device is needed.

The GPU cases of tests/test_gpu_far_rows.py rest on one claim: whatever address a 32-bit slip in a kernel's or the
host's `row * stride` produces for row 1, it lies INSIDE the arena and NOT in row 1 -- on a guard or on row 0 -- so the
slip shows as a failed assertion (a guard written, row 0 overwritten, row 1 left as the sentinel, row 0's data read
twice) and cannot leave the allocation.  This file holds that claim for every dtype, every row length of the grid and
every truncation model; no mutant kernel is run on a device for it."""
import numpy as np
import pytest
import torch

import row_windows as rw
from row_windows import EXTRA, FAR_DTYPES, FAR_STRIDE, LEFT
from waveforms_amd import _rows

NS = [1, 15, 4097, 20011]
# what a slip cuts to 32 bits: the offset of row 1 in elements (then scaled to bytes at full width) or in bytes; as
# int32 or as uint32
MODELS = [(unit, signed) for unit in ('element', 'byte') for signed in (True, False)]


def _cut(v, signed):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if signed and v >= 1 << 31 else v


def _slipped(offset_elems, es, unit, signed):
    """byte offset from row 0's first sample that the slip gives for the element `offset_elems` past it"""
    return _cut(offset_elems, signed) * es if unit == 'element' else _cut(offset_elems * es, signed)


def test_the_constants():
    assert FAR_STRIDE == 2**32 + 37 and FAR_STRIDE % 2 == 1 and (LEFT, EXTRA) == (5, 37)
    assert [np.dtype(d).name for d in FAR_DTYPES] == ['float64', 'float32', 'complex64', 'int16']
    assert rw.far_arena_elems(100) == LEFT + FAR_STRIDE + 100 + EXTRA
    assert rw.FAR_ARENA_BYTES == rw.far_arena_elems(rw.FAR_MAX_N) * 8 and max(NS) <= rw.FAR_MAX_N
    assert 34.3e9 < rw.FAR_ARENA_BYTES < 34.5e9
    # the truncated offsets the module's comment names
    assert _cut(FAR_STRIDE, True) == _cut(FAR_STRIDE, False) == 37
    assert {np.dtype(d).name: _cut(FAR_STRIDE * np.dtype(d).itemsize, True) for d in FAR_DTYPES} == \
        {'float64': 296, 'float32': 148, 'complex64': 296, 'int16': 74}


@pytest.mark.parametrize('unit,signed', MODELS, ids=[f'{u}_{"int32" if s else "uint32"}' for u, s in MODELS])
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('dtype', FAR_DTYPES, ids=[np.dtype(d).name for d in FAR_DTYPES])
def test_a_32_bit_slip_stays_inside_the_arena_and_shows(dtype, n, unit, signed):
    es = np.dtype(dtype).itemsize
    arena = rw.far_arena_elems(n) * es                                     # bytes; the arena starts at address 0 here
    row0 = (LEFT * es, (LEFT + n) * es)
    row1 = ((LEFT + FAR_STRIDE) * es, (LEFT + FAR_STRIDE + n) * es)
    assert row1[1] + EXTRA * es == arena and arena <= rw.FAR_ARENA_BYTES
    # the first and the last sample of row 1: `row * stride` cut alone, and `row * stride + i` cut as a whole
    for i, whole in ((0, False), (n - 1, False), (n - 1, True)):
        true = row1[0] + i * es
        got = row0[0] + (_slipped(FAR_STRIDE + i, es, unit, signed) if whole
                         else _slipped(FAR_STRIDE, es, unit, signed) + i * es)
        assert 0 <= got and got + es <= arena, (got, arena)                # inside the allocation: no fault
        assert got != true                                                 # and wrong
        assert not (row1[0] <= got < row1[1])                              # on a guard or on row 0: the tests see it
        in_row0 = row0[0] <= got < row0[1]
        in_guard = got < row0[0] or row0[1] <= got < row1[0] or got >= row1[1]
        assert in_row0 != in_guard
        assert got % es == 0                                               # a whole element of the dtype, as the scan counts


def test_a_stride_between_2_pow_31_and_2_pow_32_would_leave_the_allocation():
    """why the stride is not smaller: the int32 slip of such a stride is negative, in front of row 0 and of the arena"""
    for stride in (2**31 + 37, 2**32 - 37):
        for dtype in FAR_DTYPES:
            es = np.dtype(dtype).itemsize
            assert LEFT * es + _slipped(stride, es, 'element', True) < 0


@pytest.mark.parametrize('es', [2, 4, 8])
@pytest.mark.parametrize('n', NS)
def test_disjointness_of_far_extents(n, es):
    """`rows_disjoint` on plain tuples: extents ((batch - 1) * stride + n) * itemsize beyond 2^35 bytes"""
    base, batch = 1 << 21, 2
    extent = ((batch - 1) * FAR_STRIDE + n) * es
    assert extent > 2**32 * es and (es < 8 or extent > 2**35)
    far = (base, FAR_STRIDE, batch, n, es)

    def disjoint(a, b):
        ab, ba = _rows.rows_disjoint(a, b), _rows.rows_disjoint(b, a)
        assert ab == ba
        return ab

    # near rows anywhere inside the far extent meet it: at its start, between the two rows, on row 1, on its last element
    for at in (base, base + n * es, base + 2**32, base + FAR_STRIDE * es, base + extent - es):
        assert not disjoint(far, (at, n, 1, n, es)), at
    assert not disjoint(far, (base + extent - es, FAR_STRIDE, batch, n, es))     # two far batches sharing one element
    assert not disjoint(far, (base + 37 * es, FAR_STRIDE, batch, n, es))         # interleaved far batches: extents meet
    # extents that only touch, on either side, and extents apart
    assert disjoint(far, (base + extent, n, batch, n, es))
    assert disjoint(far, (base + extent, FAR_STRIDE, batch, n, es))
    assert disjoint(far, (base - batch * n * es, n, batch, n, es))
    assert disjoint(far, (base + extent + es, FAR_STRIDE, batch, n, es))
    # the extent ends at the END of row 1, not at batch * stride
    assert extent < batch * FAR_STRIDE * es
    # rows of no samples occupy nothing
    assert disjoint((base, FAR_STRIDE, batch, 0, es), (base, FAR_STRIDE, batch, 0, es))


@pytest.mark.parametrize('npdt', [np.float64, np.float32, np.int16], ids=['float64', 'float32', 'int16'])
@pytest.mark.parametrize('n', NS)
def test_check_rows_accepts_the_far_stride(n, npdt):
    """a meta tensor has the metadata and no memory: every clause of `check_rows` reads it as it would a device tensor's
    (`device=False` leaves the "is a device tensor" clause out; a meta tensor's data_ptr() is 0)"""
    tdt = _rows.torch_dtype(npdt)
    t = torch.empty_strided((2, n), (FAR_STRIDE, 1), dtype=tdt, device='meta')
    assert _rows.check_rows(t, 2, n, tdt, 'refused', device=False) == (t.data_ptr(), FAR_STRIDE)
    assert _rows.check_rows(t, None, n, None, 'refused', exact=True, device=False)[1] == FAR_STRIDE
    for bad_rows, bad_n, kw in ((3, n, {}), (2, n + 1, {}), (2, n - 1, {'exact': True})):
        with pytest.raises(ValueError, match='refused'):
            _rows.check_rows(t, bad_rows, bad_n, tdt, 'refused', device=False, **kw)
    with pytest.raises(ValueError, match='refused'):                        # the device clause, switched on
        _rows.check_rows(t, 2, n, tdt, 'refused')
    # one far row: its stride(0) means nothing, and is >= n, so it goes down as it is
    one = torch.empty_strided((1, n), (FAR_STRIDE, 1), dtype=tdt, device='meta')
    assert _rows.check_rows(one, 1, n, tdt, 'refused', device=False)[1] == FAR_STRIDE
