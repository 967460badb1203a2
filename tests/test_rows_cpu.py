"""The row rule of every stage that takes "a batch of rows" (waveforms_amd/_rows.py; DESIGN.md, "The row rule"), on CPU
tensors with the "is a device tensor" clause switched off: every clause of the row check and of the state check, the
disjointness rule as integers (the cases tests/test_gpu_fir_pipeline.py::test_overlapping_out_is_refused spells out),
and the context managers of the owners.  No device, no library load."""
import ctypes as C

import numpy as np
import pytest
import torch

from waveforms_amd import _engine, _rows

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32), (np.int16, torch.int16)]
MSG = 'the text of this call site'


def rows_tensor(batch, n, stride, tdt):
    """(batch, n) windows at column 0 of a (batch, stride) tensor"""
    return torch.zeros((batch, stride), dtype=tdt)[:, :n]


def check(t, rows, n, tdt, **kw):
    return _rows.check_rows(t, rows, n, tdt, MSG, device=False, **kw)


@pytest.mark.parametrize('npdt,tdt', DTYPES)
def test_dtype_map(npdt, tdt):
    assert _rows.torch_dtype(npdt) is tdt and _rows.torch_dtype(np.dtype(npdt)) is tdt


@pytest.mark.parametrize('npdt,tdt', DTYPES)
@pytest.mark.parametrize('pad', [0, 2])
@pytest.mark.parametrize('n', [0, 1, 5])
@pytest.mark.parametrize('batch', [1, 3])
def test_accepted_rows(batch, n, pad, npdt, tdt):
    t = rows_tensor(batch, n, n + pad, tdt)
    want = (t.data_ptr(), max(n + pad, 1))                                   # (torch: a row of no elements has stride 1)
    assert check(t, batch, n, _rows.torch_dtype(npdt)) == want
    assert check(t, None, n, tdt) == want                                    # any number of rows
    assert check(t, batch, n, None) == want                                  # any dtype
    assert check(t, batch, n, tdt, exact=True) == want
    if n:
        assert check(t, batch, n - 1, tdt) == want                           # wider than asked
    # a window x[:, 3:3 + n] of a wider tensor: the wide stride, the window's address
    wide = torch.zeros((batch, n + 7), dtype=tdt)
    win = wide[:, 3:3 + n]
    assert check(win, batch, n, tdt) == (win.data_ptr(), n + 7)
    if n:                                                                    # (torch gives an empty window no address)
        assert win.data_ptr() == wide.data_ptr() + 3 * wide.element_size()


@pytest.mark.parametrize('npdt,tdt', DTYPES)
def test_every_clause_refuses(npdt, tdt):
    batch, n = 3, 5
    good = rows_tensor(batch, n, n + 2, tdt)
    other = torch.float32 if tdt is not torch.float32 else torch.float64
    bad = {
        'dtype': (good.to(other), batch, n, {}),
        'not 2-D': (good[0], batch, n, {}),
        '3-D': (good[None], batch, n, {}),
        'row count': (good, batch + 1, n, {}),
        'too narrow': (good, batch, n + 1, {}),
        'not exactly n wide': (good, batch, n - 1, {'exact': True}),
        'stride(1) != 1': (torch.zeros((batch, 2 * n), dtype=tdt)[:, ::2], batch, n, {}),
        'stride(0) < n': (torch.zeros(n + batch, dtype=tdt).as_strided((batch, n), (1, 1)), batch, n, {}),
        'stride(0) == 0': (torch.zeros((1, n), dtype=tdt).expand(batch, n), batch, n, {}),
    }
    check(good, batch, n, tdt)
    for what, (t, rows, want_n, kw) in bad.items():
        with pytest.raises(ValueError, match=MSG):
            check(t, rows, want_n, tdt, **kw)
            pytest.fail(f'{what}: accepted')
    # the device clause, switched on: a CPU tensor is refused
    with pytest.raises(ValueError, match=MSG):
        _rows.check_rows(good, batch, n, tdt, MSG)


@pytest.mark.parametrize('npdt,tdt', DTYPES)
def test_one_row_and_one_element_rows(npdt, tdt):
    n = 5
    # one row: stride(0) means nothing, n goes down in its place
    for stride0 in (0, 1, n - 1):
        t = torch.zeros(n, dtype=tdt).as_strided((1, n), (stride0, 1))
        assert check(t, 1, n, tdt) == (t.data_ptr(), n)
    # rows one element wide: stride(1) means nothing
    col = torch.zeros((3, 4), dtype=tdt).t()[:, :1]                          # shape (4, 1), strides (1, 4)
    assert col.stride(1) != 1
    assert check(col, 4, 1, tdt) == (col.data_ptr(), 1)
    assert check(col, 4, 0, tdt) == (col.data_ptr(), 1)
    with pytest.raises(ValueError):                                          # two elements wide: it counts again
        check(torch.zeros((3, 8), dtype=tdt).t()[:, :2], 8, 1, tdt)


def test_state_check():
    rows, D = 3, 4
    good = torch.zeros((rows, D), dtype=torch.float64)
    assert _rows.check_state(None, (rows, D), MSG, device=False) is None
    assert _rows.check_state(None, (rows, D), MSG) is None
    assert _rows.check_state(good, (rows, D), MSG, device=False) == good.data_ptr()
    assert _rows.check_state(good[0], (D, ), MSG, device=False) == good.data_ptr()       # one level per row: 1-D
    for bad in (good.float(), good[:2], good[:, :3], torch.zeros((rows, 2 * D), dtype=torch.float64)[:, ::2],
                good.reshape(-1), torch.zeros((D, rows), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match=MSG):
            _rows.check_state(bad, (rows, D), MSG, device=False)
    with pytest.raises(ValueError, match=MSG):
        _rows.check_state(good, (rows, D), MSG)                              # a CPU tensor with the device clause on


@pytest.mark.parametrize('es', [4, 8])
@pytest.mark.parametrize('n,batch', [(1000, 3), (5, 3), (5, 1), (1, 3)])
def test_disjointness(n, batch, es):
    base = 1 << 20

    def disjoint(a_ptr, b_ptr, a_stride=n, b_stride=n, n_=n):
        a, b = (a_ptr, a_stride, batch, n_, es), (b_ptr, b_stride, batch, n_, es)
        ab, ba = _rows.rows_disjoint(a, b), _rows.rows_disjoint(b, a)
        assert ab == ba                                                      # either way round
        return ab

    extent = ((batch - 1) * n + n) * es
    # the identical range, one row on, 8 bytes on, one shared element
    for shift in (0, n * es, 8, extent - es):
        if shift < extent:
            assert not disjoint(base, base + shift), shift
    # ranges that only touch, and ranges apart
    assert disjoint(base, base + extent)
    assert disjoint(base, base + extent + es)
    # strided rows: the extent runs to the END of the last row, not to batch * stride
    stride = n + 7
    end = ((batch - 1) * stride + n) * es
    assert not disjoint(base, base + end - es, a_stride=stride)
    assert disjoint(base, base + end, a_stride=stride)
    assert end < batch * stride * es
    # rows of no samples occupy nothing
    assert disjoint(base, base, n_=0)
    assert disjoint(base, base + 8, a_stride=0, b_stride=0, n_=0)


class _CountingHandle(_engine._Handle):
    closes = 0

    def close(self):
        self.closes += 1


class _CountingBuffer(_engine.DeviceBuffer):
    closes = 0

    def __init__(self):                                                      # (no allocation: no library)
        self.ptr = None

    def close(self):
        self.closes += 1


@pytest.mark.parametrize('cls', [_CountingHandle, _CountingBuffer])
def test_owners_are_context_managers(cls):
    with cls() as h:
        assert isinstance(h, cls) and h.closes == 0
    assert h.closes == 1
    with pytest.raises(KeyError):
        with cls() as h:
            raise KeyError('inside the block')
    assert h.closes == 1


def test_plain_owners_close_without_a_library():
    """a handle that holds nothing and a buffer that holds nothing: the block ends without a library call"""
    with _engine._Handle() as h:
        assert not h._h
    assert isinstance(h._h, C.c_void_p) and not h._h
    b = _engine.DeviceBuffer.__new__(_engine.DeviceBuffer)
    with b as inside:
        assert inside is b
    assert getattr(b, 'ptr', None) is None
