"""Rows as a window of a wider device tensor, with guard bands ("The row rule").

A stage that takes `(ptr, stride)` rows must write the n samples of each row and nothing else.  `Window` builds a
wide `(rows + 2, n + 37)` tensor filled with a sentinel bit pattern and hands out the window
`wide[1:1 + rows, 5:5 + n]`: an odd element offset and an odd row stride, so there is no 16-byte alignment to lean
on; the guard row above catches a write before row 0, the one below a write after the last row, the columns left and
right a write past either end of a row.  Guards are compared through an integer view, so the sentinel (a NaN with a
payload: arithmetic on it would show as well) needs no value semantics.  A plain module like golden_io.py."""
import numpy as np

GUARD_ROWS, LEFT, EXTRA = 1, 5, 37
_SENTINEL = {4: 0x7FC5A5A5, 8: 0x7FF8A5A5A5A5A5A5}     # per real component: float32 | float64 quiet NaNs with a payload


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32,
            np.dtype(np.complex128): torch.complex128, np.dtype(np.complex64): torch.complex64}[np.dtype(dtype)]


def _int_view(t):
    """the tensor's bits: int32 / int64 per real component (a complex tensor gets a trailing axis of 2)"""
    import torch
    r = torch.view_as_real(t) if t.is_complex() else t
    return r.view(torch.int32 if r.element_size() == 4 else torch.int64)


class Window:
    """`rows` rows of `n` elements of NumPy dtype `dtype` (float64, float32, complex128, complex64) inside a wide
    sentinel-filled tensor; `values` (rows, n), if given, are written into the window.

        .win      the window, a torch view: pass it to *_torch entry points
        .ptr      its data pointer, .stride its row stride in elements of `dtype`: pass them to raw plans"""

    def __init__(self, rows, n, dtype, values=None):
        import torch
        self.rows, self.n, self.dtype = int(rows), int(n), np.dtype(dtype)
        self.wide = torch.empty((self.rows + 2 * GUARD_ROWS, self.n + EXTRA), dtype=_torch_dtype(dtype), device='cuda')
        bits = _int_view(self.wide)
        self.sentinel = _SENTINEL[bits.element_size()]
        bits.fill_(self.sentinel)
        self.win = self.wide[GUARD_ROWS:GUARD_ROWS + self.rows, LEFT:LEFT + self.n]
        self.ptr, self.stride = self.win.data_ptr(), self.wide.stride(0)
        if values is not None:
            self.put(values)

    def put(self, values):
        import torch
        v = np.array(np.broadcast_to(np.asarray(values, dtype=self.dtype), (self.rows, self.n)))     # (a writeable copy)
        self.win.copy_(torch.from_numpy(v).cuda())

    def host(self):
        """the window's content, a contiguous (rows, n) host array"""
        return self.win.contiguous().cpu().numpy()

    def guards_intact(self):
        """-> None when every element outside the window still holds the sentinel's bits, else a message naming the
        first few (row, column) of the WIDE tensor that were written"""
        import torch
        bits = _int_view(self.wide)
        hit = bits != self.sentinel
        if hit.dim() == 3:
            hit = hit.any(dim=2)
        hit[GUARD_ROWS:GUARD_ROWS + self.rows, LEFT:LEFT + self.n] = False
        if not bool(hit.any()):
            return None
        where = torch.nonzero(hit)[:6].cpu().tolist()
        return (f'{int(hit.sum())} guard elements written; first at (row, column) of the wide tensor {where} '
                f'(window: rows {GUARD_ROWS}..{GUARD_ROWS + self.rows - 1}, columns {LEFT}..{LEFT + self.n - 1})')

    def assert_guards(self):
        msg = self.guards_intact()
        assert msg is None, msg

    def assert_holds(self, values):
        """the window is bit for bit `values` and the guards are intact: an input that an out-of-place apply left alone"""
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=self.dtype), (self.rows, self.n)))
        assert bits_equal(self.host(), v), 'the window no longer holds what was put there'
        self.assert_guards()


def bits_equal(a, b):
    """two host arrays of one dtype and shape, bit for bit (so that -0.0 != 0.0 and a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
