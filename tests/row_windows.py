"""Rows as a window of a wider device tensor, with guard bands ("The row rule").

A stage that takes `(ptr, stride)` rows must write the n samples of each row and nothing else.  `Window` builds a
wide `(rows + 2, n + 37)` tensor filled with a sentinel bit pattern and hands out the window
`wide[1:1 + rows, 5:5 + n]`: an odd element offset and an odd row stride, so there is no 16-byte alignment to lean
on; the guard row above catches a write before row 0, the one below a write after the last row, the columns left and
right a write past either end of a row.  Guards are compared through an integer view, so the sentinel (a NaN with a
payload: arithmetic on it would show as well) needs no value semantics.  A plain module like golden_io.py.

`FarWindow` is the same thing with two rows MORE THAN 2^32 ELEMENTS APART: the corner of the row rule (any stride >= n)
at which a `row * stride` computed in 32 bits goes wrong.  It has the interface of `Window`, so a case can take either."""
import numpy as np

GUARD_ROWS, LEFT, EXTRA = 1, 5, 37
# per real component: float32 | float64 quiet NaNs with a payload; int16 codes: 0xA5C3
_SENTINEL = {2: -23101, 4: 0x7FC5A5A5, 8: 0x7FF8A5A5A5A5A5A5}

# Why this stride.  An element offset of 2^32 + 37 cut to int32 or uint32 is 37; its byte offset cut the same way is 296
# (float64, complex64), 148 (float32) or 74 (int16).  Every address a 32-bit slip can produce is therefore non-negative and
# inside the arena, at or near row 0: a wrong store lands on a guard or on row 0, a wrong read returns row 0 or the
# sentinel -- a failed assertion, never a device fault.  (A stride between 2^31 and 2^32 would make the int32 slip negative,
# in front of the allocation.)  Odd, so there is no alignment to lean on.  tests/test_far_rows_cpu.py holds this arithmetic.
FAR_STRIDE = 2**32 + 37
FAR_ROWS = 2
FAR_MAX_N = 1 << 17                                    # the longest far row; the arena is sized for it
FAR_DTYPES = (np.float64, np.float32, np.complex64, np.int16)
_SLAB_BYTES = 1 << 29                                  # the guard scan looks at this much of the arena at a time


def far_arena_elems(n):
    """elements of the flat arena around two far rows of n elements"""
    return LEFT + FAR_STRIDE + int(n) + EXTRA


FAR_ARENA_BYTES = far_arena_elems(FAR_MAX_N) * 8       # 34.4 GB: float64 / complex64 rows; the other dtypes use a prefix
_far = {'bytes': None, 'live': None}


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32,
            np.dtype(np.complex128): torch.complex128, np.dtype(np.complex64): torch.complex64,
            np.dtype(np.int16): torch.int16}[np.dtype(dtype)]


def _int_view(t):
    """the tensor's bits: int32 / int64 per real component (a complex tensor gets a trailing axis of 2); int16 as it is"""
    import torch
    r = torch.view_as_real(t) if t.is_complex() else t
    return r.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[r.element_size()])


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


def free_far_arena():
    """drop the far arena and hand its memory back to the device: without this the caching allocator keeps 34 GB for the
    rest of the process.  A `FarWindow` made before is dead afterwards."""
    import gc
    import torch
    _far['bytes'] = _far['live'] = None
    gc.collect()
    torch.cuda.empty_cache()


def _far_bytes():
    import torch
    if _far['bytes'] is None:
        _far['bytes'] = torch.empty(FAR_ARENA_BYTES, dtype=torch.uint8, device='cuda')
    return _far['bytes']


class FarWindow:
    """Two rows of `n` elements of NumPy dtype `dtype` (float64, float32, complex64, int16), FAR_STRIDE elements apart,
    in a flat sentinel-filled arena of `far_arena_elems(n)` elements; row 0 starts LEFT elements into it.  The interface
    of `Window` (.win, .ptr, .stride, put, host, guards_intact, assert_guards, assert_holds).

    complex128 is left out: its arena would be 68.7 GB; float64 covers the 8-byte element path and complex64 the complex
    one.  One arena per process, made on first use as bytes sized for float64 and viewed per dtype; making a FarWindow
    refills it with the sentinel, so AT MOST ONE is alive at a time (the other side of an out-of-place case is an
    ordinary `Window`): an older one refuses to be used.  `free_far_arena()` gives the memory back."""
    rows = FAR_ROWS

    def __init__(self, n, dtype, values=None):
        self.n, self.dtype = int(n), np.dtype(dtype)
        assert 1 <= self.n <= FAR_MAX_N and self.dtype in [np.dtype(d) for d in FAR_DTYPES], (n, dtype)
        self.elems = far_arena_elems(self.n)
        self.arena = _far_bytes()[:self.elems * self.dtype.itemsize].view(_torch_dtype(dtype))
        _far['live'] = self
        bits = _int_view(self.arena)
        self.sentinel = _SENTINEL[bits.element_size()]
        bits.fill_(self.sentinel)
        self.win = self.arena.as_strided((FAR_ROWS, self.n), (FAR_STRIDE, 1), self.arena.storage_offset() + LEFT)
        self.ptr, self.stride = self.win.data_ptr(), FAR_STRIDE
        assert self.ptr == self.arena.data_ptr() + LEFT * self.dtype.itemsize and self.win.stride(0) == FAR_STRIDE
        if values is not None:
            self.put(values)

    def _alive(self):
        assert _far['live'] is self, 'a later FarWindow (or free_far_arena) has taken the arena'

    def put(self, values):
        import torch
        self._alive()
        v = np.array(np.broadcast_to(np.asarray(values, dtype=self.dtype), (FAR_ROWS, self.n)))     # (a writeable copy)
        for r in range(FAR_ROWS):                      # row by row: each is a plain contiguous 1-D copy
            self.win[r].copy_(torch.from_numpy(v[r]).cuda())

    def host(self):
        """the window's content, a contiguous (2, n) host array"""
        self._alive()
        return np.stack([self.win[r].cpu().numpy() for r in range(FAR_ROWS)])

    def _scan(self, want_where):
        """-> (number of arena elements outside the two rows that no longer hold the sentinel, the first few offsets);
        through the integer view, a slab at a time so that the temporaries stay far below 1 GiB"""
        import torch
        bits = _int_view(self.arena).reshape(-1)
        comps = bits.numel() // self.elems                                  # 2 for complex64
        slab = _SLAB_BYTES // bits.element_size()                          # (a whole number of elements: a power of two)
        keep = [((LEFT + r * FAR_STRIDE) * comps, (LEFT + r * FAR_STRIDE + self.n) * comps) for r in range(FAR_ROWS)]
        total, where = torch.zeros((), dtype=torch.int64, device='cuda'), []
        for lo in range(0, bits.numel(), slab):
            hi = min(lo + slab, bits.numel())
            hit = bits[lo:hi] != self.sentinel
            for a, b in keep:
                if a < hi and lo < b:
                    hit[max(a, lo) - lo:min(b, hi) - lo] = False
            if comps > 1:                                                   # an element is written if a component is
                hit = hit.view(-1, comps).any(dim=1)
            if want_where and len(where) < 6 and bool(hit.any()):
                first = int(hit.to(torch.uint8).argmax())                   # then the hits among the 4096 elements from it
                near = torch.nonzero(hit[first:first + 4096])[:, 0].cpu().tolist()
                where += [lo // comps + first + i for i in near]
            total += hit.count_nonzero()
        return int(total), where[:6]

    def guards_intact(self):
        """-> None when every element of the arena outside the two rows still holds the sentinel's bits, else a message
        naming the first few arena offsets (in elements) that were written"""
        self._alive()
        if self._scan(False)[0] == 0:
            return None
        count, where = self._scan(True)
        return (f'{count} guard elements written; first at arena offsets {where} (rows: {LEFT}..{LEFT + self.n - 1} '
                f'and {LEFT + FAR_STRIDE}..{LEFT + FAR_STRIDE + self.n - 1})')

    def assert_guards(self):
        msg = self.guards_intact()
        assert msg is None, msg

    def assert_holds(self, values):
        """the two rows are bit for bit `values` and the guards are intact: an input that an out-of-place apply left alone"""
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=self.dtype), (FAR_ROWS, self.n)))
        assert bits_equal(self.host(), v), 'the far rows no longer hold what was put there'
        self.assert_guards()


def bits_equal(a, b):
    """two host arrays of one dtype and shape, bit for bit (so that -0.0 != 0.0 and a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
