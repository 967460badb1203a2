"""The row rule of every stage that takes "a batch of rows", spelt once ("The row rule"); the C side of
it is csrc/wfk_host.h.  Checks on tensor metadata only: nothing here touches the device or loads the library."""
from __future__ import annotations

import numpy as np


_TORCH = {}


def torch_dtype(dtype):
    """the torch dtype of a plan's NumPy dtype: float64 / float32 rows, int16 codes (the demodulator's input, the DAC
    stage's output), the DAC and marker stages' int64 counts, the marker stage's uint8 markers, the segment stage's
    int32 table and the demodulator's complex128 result"""
    if not _TORCH:
        import torch
        _TORCH.update({np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32,
                       np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32,
                       np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8,
                       np.dtype(np.complex128): torch.complex128})
    return _TORCH[np.dtype(dtype)]


def check_rows(t, rows, n, dtype, message, exact=False, device=True):
    """`t` is a 2-D device tensor of the torch dtype `dtype` (None: any) with `rows` rows (None: any number) of >= n
    elements (`exact`: of n), unit stride along a row that has more than one element, and -- more than one row -- a
    row stride >= n: ValueError(message) otherwise.  -> (data_ptr, the row stride to pass down); a single row's stride(0) means
    nothing, so n stands in for one below it.  `device=False` leaves the "is a device tensor" clause out."""
    if ((device and not t.is_cuda) or (dtype is not None and t.dtype != dtype) or t.dim() != 2
            or (rows is not None and t.shape[0] != rows) or (t.shape[1] != n if exact else t.shape[1] < n)
            or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < n)):
        raise ValueError(message)
    return t.data_ptr(), max(t.stride(0), n)


def check_state(z, shape, message, device=True, dtype=np.float64):
    """what goes with the rows -- zi / zf (rows, state_dim), levels (rows,), the DAC stage's int64 counts (rows, 3):
    None, or a contiguous device tensor of that shape and of `dtype` (float64 unless given; ValueError(message)
    otherwise) -> None or its data_ptr"""
    if z is None:
        return None
    if ((device and not z.is_cuda) or z.dtype != torch_dtype(dtype) or not z.is_contiguous()
            or tuple(z.shape) != tuple(shape)):
        raise ValueError(message)
    return z.data_ptr()


def rows_disjoint(a, b) -> bool:
    """a, b: (ptr, row stride, batch, n, itemsize) of two row batches.  A batch occupies the bytes from the first
    sample of row 0 to the END of row batch - 1 (not batch * stride); two batches are disjoint when these half-open
    ranges do not meet.  Rows of no samples occupy nothing.  (RowSide::bytes / wfk_ranges_overlap of wfk_row_rule.h)"""
    a0, a_stride, a_batch, a_n, a_es = a
    b0, b_stride, b_batch, b_n, b_es = b
    return a_n == 0 or b_n == 0 or not (a0 < b0 + ((b_batch - 1) * b_stride + b_n) * b_es
                                        and b0 < a0 + ((a_batch - 1) * a_stride + a_n) * a_es)


def report_disjoint(ptr, rows, counters, *sides) -> bool:
    """the contiguous int64 report of `rows` x `counters` at `ptr` (None: no report) meets none of `sides`, tuples as
    rows_disjoint takes them  (RowReport of wfk_row_rule.h)"""
    if ptr is not None:
        report = (ptr, counters, rows, counters, 8)
        for side in sides:
            if not rows_disjoint(report, side):
                return False
    return True
