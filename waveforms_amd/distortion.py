"""Pre-distortion stages on the GPU: `predistort(sig, filters=..., ker=...)`.

Signature and semantics follow the reference's `predistort`
(waveforms/distortion.py:289-337):
  * FIR branch (`ker=`): out[i] = sum_k ker[k] * sig[i + len(ker)//2 - k], zero padded --
    what the reference computes with one giant `scipy.signal.fftconvolve`;
  * IIR branch (`filters=`): the combined transfer function run as
    `scipy.signal.lfilter(b, a, sig, zi=lfiltic(...))` -- here a
    block-parallel linear-recurrence scan (csrc/wfk_iir.hip).
Filter *design* (polynomial products, zpk conversions: O(order) host work, never per
sample) uses NumPy/SciPy exactly as the reference does.
"""
from __future__ import annotations

import contextlib
import warnings

import numpy as np

from . import _engine, _rows


class FirStage:
    """Device-resident FIR stage for `batch` rows of `n` samples (build once, apply
    many times).  `apply_torch(x, y)`: x, y (batch, >= n) device tensors.  `ker` of shape (batch, K):
    one kernel per row."""

    def __init__(self, ker, n: int, batch: int = 1, dtype=np.float64):
        self.plan = _engine.FirPlan(ker, n, batch, dtype)
        self.n, self.batch, self.dtype = int(n), int(batch), np.dtype(dtype)

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, stream=0):
        self.plan.apply(in_ptr, in_stride, out_ptr, out_stride, stream)

    def kernel_name(self) -> str:
        """the form the stage runs (`_engine.FirPlan.kernel_name`)"""
        return self.plan.kernel_name()

    def apply_torch(self, x, y):
        import torch
        (x0, xs), (y0, ys) = (_rows.check_rows(
            t, self.batch, self.n, _rows.torch_dtype(self.dtype),
            'expected (batch, >=n) row-contiguous device tensors of the plan dtype') for t in (x, y))
        es = self.dtype.itemsize
        if not _rows.rows_disjoint((x0, xs, self.batch, self.n, es), (y0, ys, self.batch, self.n, es)):
            raise ValueError('FIR is out of place: y overlaps x')
        self.apply(x0, xs, y0, ys, torch.cuda.current_stream(x.device).cuda_stream)
        return y

    def close(self):
        self.plan.close()


def _row_state(z, r, own_orders, section_order):
    """row r's own state out of a (rows, state_dim) host array of per-row cascades padded to a common shape
    (`_engine.pack_sections_rows`): section s sits at s * section_order and is own_orders[r][s] long"""
    z, m = np.asarray(z), section_order
    return np.concatenate([z[r, s * m:s * m + o] for s, o in enumerate(own_orders[r])] or [z[r, :0]])


def _initial_host(initial, rows, message):
    """a scalar (every row) or one value per row -> (rows,) float64 array; ValueError(message) for any other shape"""
    arr = np.asarray(initial, dtype=np.float64)
    if arr.ndim == 0:
        arr = np.full(rows, float(arr))
    if arr.shape != (rows, ):
        raise ValueError(message)
    return arr


def _initial_rows(owner, rows, initial, device):
    """the per-row `initial` of a stage: a scalar, one value per row, or a (rows,) float64 device tensor -> None (all
    zero) or a (rows,) float64 device tensor; a tensor of the last values is kept in `owner._initial_cache`"""
    import torch
    if isinstance(initial, torch.Tensor):
        _rows.check_state(initial, (rows, ), 'initial: a (batch,) contiguous float64 device tensor')
        return initial
    arr = _initial_host(initial, rows, 'initial: a scalar or one value per row')
    if not arr.any():
        return None
    c = owner._initial_cache
    if c is None or c[1] != device or not np.array_equal(c[0], arr):
        owner._initial_cache = c = (arr.copy(), device, torch.from_numpy(arr.copy()).to(device))
    return c[2]


# what a stage calls its rows -> the refusals of its counts, its beyond and its zi / zf, ready made: an apply formats nothing
_FRONT_TEXTS = {who: (f'expected counts: contiguous ({who}, 3) int64 device tensor',
                      f'expected beyond: contiguous ({who}, 3) int64 device tensor',
                      f'zi / zf must be contiguous ({who}, state_dim) float64 device tensors')
                for who in ('batch', 'rows_out', 'n_channels')}


def _state_ptrs(zi, zf, rows, state_dim, rows_name):
    """the optional zi / zf of a stage with state, (rows, state_dim) float64 device tensors, -> (zi pointer or None,
    zf pointer or None); `rows_name`: what the refusal calls the rows ('batch', 'n_channels')"""
    if zi is None and zf is None:
        return None, None
    message = _FRONT_TEXTS[rows_name][2]
    return _rows.check_state(zi, (rows, state_dim), message), _rows.check_state(zf, (rows, state_dim), message)


class IirStage:
    """Device-resident IIR stage for `batch` rows of `n` samples (build once, apply many times), the
    counterpart of `FirStage`:  y[r] = F_r(x[r] - initial[r]) + initial[r].

    `sections` is either ONE cascade for all rows -- a list of (b, a) pairs or an SOS matrix (n_sections, 6);
    it runs on `_engine.IirPlan`, results as ever -- or a list of `batch` cascades, one list of (b, a) pairs
    per row (`per_row`; `_engine.IirRowsPlan`, one launch for the whole batch).  Per-row cascades are padded
    with zero coefficients to a common shape, which must be sections of equal order with a total state
    dimension <= 4 (NotImplementedError otherwise, the message names the limit).

        st = IirStage([[exp_decay_filter(A, tau, 2e9)] for A, tau in lines], n, len(lines))
        st.apply_torch(x)                      # in place, on torch's current stream
        st.apply_torch(x, out=y, initial=levels, zi=zi, zf=zf)

    zi / zf: (batch, state_dim) float64 device tensors in scipy's layout per row.  With per-row cascades
    `state_dim` is that of the common shape; `row_state(zf, r)` cuts row r's own state out of it (the padding
    entries are zero)."""

    def __init__(self, sections, n: int, batch: int, dtype=np.float64):
        self.n, self.batch, self.dtype = int(n), int(batch), np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError('IirStage: dtype must be float64 or float32')
        if self.batch < 1 or self.n < 0:
            raise ValueError('IirStage: batch >= 1 and n >= 0')
        cascades, shared = _cascade_rows('IirStage', sections, self.batch,
                                         '[(b, a), ...], an SOS matrix, or one [(b, a), ...] per row')
        self.per_row = shared is None
        self._initial_cache = None
        if self.per_row:
            self.plan = _engine.IirRowsPlan(cascades, self.n, self.dtype)
            self.own_orders = self.plan.own_orders
            self.section_order = int(self.plan.orders[0])
        else:
            if any(np.iscomplexobj(np.asarray(c)) for sec in shared for c in sec):
                raise NotImplementedError('IIR sections with complex coefficients')
            self.plan = _engine.IirPlan(shared, self.n, self.batch, self.dtype)
        self.state_dim = self.plan.state_dim

    def kernel_name(self) -> str:
        """'iir_rows_tile<T,NSEC,ORD>' for per-row cascades; for a shared cascade what its next apply launches
        (`_engine.IirPlan.kernel_name`: 'iir_onepass<...>', 'iir_pass<...>', 'iir_scale<T>', one per pass)"""
        return self.plan.kernel_name()

    def row_state(self, z, r: int):
        """row r's own state (scipy layout, its sections back to back) out of a (batch, state_dim) host array"""
        return _row_state(z, r, self.own_orders, self.section_order) if self.per_row else np.asarray(z)[r]

    def apply_torch(self, x, out=None, initial=0.0, zi=None, zf=None):
        """x, out: (batch, >= n) row-contiguous device tensors of the stage's dtype (rows may be windows of a wider
        tensor); out=None or out is x: in place.  `initial`: a scalar, one value per row, or a (batch,) float64 device
        tensor (per-row values need per-row cascades).  Asynchronous on torch's current stream.  -> out"""
        import torch
        out = x if out is None else out
        (x0, xs), (y0, ys) = (_rows.check_rows(
            t, self.batch, self.n, _rows.torch_dtype(self.dtype),
            'expected (batch, >=n) row-contiguous device tensors of the stage dtype') for t in (x, out))
        zip_, zfp = _state_ptrs(zi, zf, self.batch, self.state_dim, 'batch')
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if self.per_row:
            ini = _initial_rows(self, self.batch, initial, x.device)
            self.plan.apply(x0, xs, y0, ys, zip_, zfp, None if ini is None else ini.data_ptr(), stream)
            return out
        if isinstance(initial, torch.Tensor) or np.ndim(initial) != 0:
            raise ValueError('a shared cascade takes a scalar `initial`; per-row levels need per-row cascades')
        for attempt in range(2):     # (a look-back timeout of the shared-cascade plan: it has switched form)
            if self.plan.apply(x0, xs, y0, ys, zip_, zfp, float(initial), stream):
                return out
        raise _engine.EngineError('IIR stage refused twice')

    def close(self):
        self.plan.close()


def _dev(stack, nbytes):
    """a device buffer of at least 8 bytes that `stack` (a contextlib.ExitStack) frees"""
    return stack.enter_context(_engine.DeviceBuffer(max(nbytes, 8)))


def _nesting(x) -> int:
    """levels of list / tuple / array around the first scalar"""
    d = 0
    while isinstance(x, (list, tuple, np.ndarray)) and len(x) > 0:
        x, d = x[0], d + 1
    return d


def _cascade_rows(who, sections, rows, spelling, one_for=None):
    """`sections` as the per-row IIR stages take it -- an SOS matrix, ONE cascade [(b, a), ...], or one cascade per
    row -- -> (one cascade per row, the ONE cascade that every row got or None).  `rows` None: the cascades decide
    the number, and ONE cascade goes to `one_for` rows.  ValueError, begun with `who`: an SOS matrix of another
    shape, another nesting ('sections is ' + `spelling`), a number of cascades that is not `rows`."""
    depth, one = _nesting(sections), None
    if depth == 2:                                             # an SOS matrix (scipy.signal.sosfilt)
        sec = np.asarray(sections, dtype=np.float64)
        if sec.ndim != 2 or sec.shape[1] != 6:
            raise ValueError(f'{who}: an SOS matrix has shape (n_sections, 6)')
        sections, depth = _engine.sos_sections(sec), 3
    if depth not in (3, 4):
        raise ValueError(f'{who}: sections is {spelling}')
    if depth == 3:                                             # one cascade: every row gets it
        one, rows = sections, one_for if rows is None else rows
        sections = [list(one)] * int(rows)
    sections = list(sections)
    if len(sections) < 1 or (rows is not None and int(rows) != len(sections)):
        raise ValueError(f'{who}: {len(sections)} cascades for {rows} rows')
    return sections, one


def _host_trip(launch, shape, dtype, rows=0, reports=(), state_dim=0, zi=None, return_zf=False, initial=None):
    """The round trip of a sampled chain's `to_host` through device buffers that live as long as the call: the result
    (`shape`, `dtype`), a (rows, 3) int64 report for every true flag in `reports`, zi and zf (rows, state_dim) where
    given / wanted, and the levels `initial` (a scalar or one per row), uploaded only where one of them is not zero.
    `launch(result, [a pointer or None per flag], zi, zf, levels)` gets the pointers (None: not there); then one
    synchronise and the downloads.  -> the result alone, or (result, the wanted reports in order, zf)"""
    D = max(state_dim, 1)
    ini = None if initial is None else np.broadcast_to(np.asarray(initial, dtype=np.float64), (rows, ))
    with contextlib.ExitStack() as stack:
        y = _dev(stack, shape[0] * shape[1] * np.dtype(dtype).itemsize)
        rep = [_dev(stack, rows * 24) if wanted else None for wanted in reports]
        dzi = _dev(stack, rows * D * 8) if zi is not None else None
        dzf = _dev(stack, rows * D * 8) if return_zf else None
        dini = _dev(stack, rows * 8) if ini is not None and ini.any() else None
        if zi is not None:
            dzi.upload(np.ascontiguousarray(np.broadcast_to(np.asarray(zi, dtype=np.float64), (rows, state_dim))))
        if dini is not None:
            dini.upload(np.ascontiguousarray(ini))
        ptr = (lambda b: None if b is None else b.ptr)
        launch(y.ptr, [ptr(r) for r in rep], ptr(dzi), ptr(dzf), ptr(dini))
        _engine.sync()
        out = [y.download(shape, dtype)] + [r.download((rows, 3), np.int64) for r in rep if r is not None]
        if return_zf:
            out.append(dzf.download((rows, D), np.float64)[:, :state_dim])
        return out[0] if len(out) == 1 else tuple(out)


class SampledFir:
    """`predistort(wav(t), ker=ker)` for many channels on one uniform grid, device-resident:
    the sampler runs INSIDE the FIR transform when the channels are fully fused (`fused`; on fine grids
    as stride-256 chains, at AWG sample rates the short tier's way: `plan.kernel_name()`), so
    the unfiltered samples never touch HBM (reference chain: waveform.py:529-563 ->
    distortion.py:329-337).  Build once, launch many times.

        sf = SampledFir(channels, ('linspace', 0.0, 3e-6, 10**7, False), ker)   # ker (K,) or (n_channels, K)
        sf.launch_torch(out)          # (n_channels, >= n) device tensor of the plan dtype
    """

    def __init__(self, channels, grid, ker, dtype=np.float64, function_lib=None, tile=1):
        """`tile` > 1 repeats the channel list that many times (synthetic batches, as BatchSampler's)"""
        from . import _flatten
        if not isinstance(grid, _flatten.wfk_grid):
            grid = _flatten.grid_from_desc(grid)
        self.prog = _flatten.tile_program(_flatten.flatten(list(channels), grid, function_lib), tile)
        self.plan = _engine.ChainPlan(self.prog, grid, ker, dtype)
        self.n, self.n_channels, self.dtype = self.plan.n, self.plan.n_channels, np.dtype(dtype)
        self.fused, self.why_not = self.plan.fused, self.plan.why_not

    def launch(self, out_ptr, out_stride=None, stream=0):
        self.plan.launch(out_ptr, self.n if out_stride is None else out_stride, stream)

    def launch_torch(self, out):
        import torch
        ptr, stride = _rows.check_rows(
            out, self.n_channels, self.n, _rows.torch_dtype(self.dtype),
            'out must be a (n_channels, >=n) row-contiguous device tensor of the plan dtype')
        self.launch(ptr, stride, torch.cuda.current_stream(out.device).cuda_stream)
        return out

    def to_host(self):
        with _engine.DeviceBuffer(max(self.n_channels * self.n, 1) * self.dtype.itemsize) as buf:
            self.launch(buf.ptr)
            _engine.sync()
            return buf.download((self.n_channels, self.n), self.dtype)

    def close(self):
        self.plan.close()


class SampledIir:
    """`sosfilt(sos, wav(t) - initial, zi) + initial` (Waveform.sample(filters=), reference waveform.py:190-203,
    244-251) -- or any cascade of (b, a) sections, optionally followed by the FIR of `predistort(., filters, ker)`
    (distortion.py:298-337) -- for many channels on one uniform grid, device-resident.  When the channels are fully
    fused and the cascade's first pass carries <= 4 state values, the wave that owns a chunk of the IIR scan evaluates
    its input itself (`fused`, `plan.kernel_name()` == 'iir_sampled<...>'): the unfiltered samples never touch HBM.

        si = SampledIir(channels, ('linspace', 0.0, 3e-6, 10**7, False), sos)        # sos (n_sections, 6) or [(b, a), ...]
        si.launch_torch(out, initial=0.0)     # (n_channels, >= n) device tensor of the plan dtype; -> final state or None
    """

    def __init__(self, channels, grid, sections, ker=None, dtype=np.float64, function_lib=None, tile=1):
        """`tile` > 1 repeats the channel list that many times (synthetic batches, as BatchSampler's)"""
        from . import _flatten
        if not isinstance(grid, _flatten.wfk_grid):
            grid = _flatten.grid_from_desc(grid)
        try:
            sec = np.asarray(sections, dtype=np.float64)
        except (ValueError, TypeError):
            sec = None
        if sec is not None and sec.ndim == 2 and sec.shape[1] == 6:
            sections = _engine.sos_sections(sec)
        self.prog = _flatten.tile_program(_flatten.flatten(list(channels), grid, function_lib), tile)
        self.plan = _engine.ChainIirPlan(self.prog, grid, sections, ker, dtype)
        self.n, self.n_channels, self.dtype = self.plan.n, self.plan.n_channels, np.dtype(dtype)
        self.state_dim = self.plan.state_dim
        self.why_not = self.plan.why_not

    @property
    def fused(self):
        return self.plan.fused

    def launch(self, out_ptr, out_stride=None, zi_ptr=None, zf_ptr=None, initial=0.0, stream=0):
        """-> False if the library refused the launch after an earlier look-back timeout (launch again)"""
        return self.plan.launch(out_ptr, self.n if out_stride is None else out_stride, zi_ptr, zf_ptr, initial, stream)

    def launch_torch(self, out, initial=0.0, zi=None, zf=None):
        """zi / zf: optional (n_channels, state_dim) float64 device tensors (initial state in / final state out)"""
        import torch
        ptr, stride = _rows.check_rows(
            out, self.n_channels, self.n, _rows.torch_dtype(self.dtype),
            'out must be a (n_channels, >=n) row-contiguous device tensor of the plan dtype')
        zip_, zfp = _state_ptrs(zi, zf, self.n_channels, self.state_dim, 'n_channels')
        s = torch.cuda.current_stream(out.device).cuda_stream
        for attempt in range(2):
            if self.launch(ptr, stride, zip_, zfp, initial, s):
                return out
        raise _engine.EngineError('IIR chain refused twice')

    def to_host(self, initial=0.0, zi=None, return_zf=False):
        """NumPy result (n_channels, n); a look-back timeout (outputs NaN) is retried once in the unfused form"""
        if np.ndim(zi) > 1:
            zi = np.asarray(zi, dtype=np.float64).reshape(-1, self.state_dim)

        def run(out, reports, dzi, dzf, levels):          # (`initial` is one scalar here: an argument, not a buffer)
            if not _engine.iir_run_checked(lambda: self.launch(out, None, dzi, dzf, initial), self.plan.status):
                raise _engine.EngineError('IIR chain failed twice')
        return _host_trip(run, shape=(self.n_channels, self.n), dtype=self.dtype, rows=self.n_channels,
                          state_dim=self.state_dim, zi=zi, return_zf=return_zf)

    def close(self):
        self.plan.close()


class SampledIirRows:
    """`predistort(wav_r(t), filters=cascade_r, initial=level_r)` for many channels on one uniform grid, every row
    its own waveform AND its own cascade (every flux line its own exp-decay correction; reference waveform.py:529-563
    -> distortion.py:100-185, 298-321), device-resident -- `BatchSampler.launch_torch(z)` followed by
    `IirStage([...one cascade per row...]).apply_torch(z)` in ONE kernel: the workgroup that owns a row evaluates each
    tile of 4096 samples in LDS and filters it there, so the unfiltered samples never touch HBM (`fused`;
    `kernel_name()` is 'iir_rows_sampled<...>' on fine grids, 'iir_rows_short<...>' at AWG sample rates).  Plans the
    fused kernels do not take (`why_not`) run the two launches.  `sections_rows`: one cascade [(b, a), ...] per
    resulting row, with `IirStage`'s per-row rules (padded to a common shape: sections of equal order, total state
    dimension <= 4).  Build once, launch many times.

        sr = SampledIirRows(channels, wl.awg_grid(n, 2e9), [[exp_decay_filter(A, tau, 2e9)] for A, tau in lines])
        sr.launch_torch(out, initial=levels, zf=zf)     # (n_channels, >= n) device tensor of the plan dtype
    """

    def __init__(self, channels, grid, sections_rows, dtype=np.float64, function_lib=None, tile=1):
        """`tile` > 1 repeats the channel list that many times (synthetic batches, as BatchSampler's)"""
        from . import _flatten
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError('SampledIirRows: dtype must be float64 or float32')
        channels, sections_rows = list(channels), list(sections_rows)
        rows = len(channels) * max(int(tile), 1)
        if len(sections_rows) != rows:
            raise ValueError(f'SampledIirRows: {len(sections_rows)} cascades for {rows} rows')
        packed = _engine.pack_sections_rows(sections_rows)         # argument errors before any device work
        if not isinstance(grid, _flatten.wfk_grid):
            grid = _flatten.grid_from_desc(grid)
        self.prog = _flatten.tile_program(_flatten.flatten(channels, grid, function_lib), tile)
        if self.prog.n_channels != rows:
            raise ValueError(f'SampledIirRows: {len(sections_rows)} cascades for {self.prog.n_channels} rows')
        self.plan = _engine.ChainIirRowsPlan(self.prog, grid, sections_rows, self.dtype, packed=packed)
        self.n, self.n_channels = self.plan.n, self.plan.n_channels
        self.state_dim = self.plan.state_dim
        self.own_orders, self.section_order = packed[3], int(packed[0][0])
        self.fused, self.why_not = self.plan.fused, self.plan.why_not
        self._initial_cache = None

    def row_state(self, z, r: int):
        """row r's own state (scipy layout, its sections back to back) out of a (n_channels, state_dim) host array"""
        return _row_state(z, r, self.own_orders, self.section_order)

    def kernel_name(self) -> str:
        """'iir_rows_sampled<T,NSEC,ORD>' | 'iir_rows_short<T,NSEC,ORD>' | '<sampler kernels> + iir_rows_tile<T,NSEC,ORD>'"""
        return self.plan.kernel_name()

    def launch(self, out_ptr, out_stride=None, zi_ptr=None, zf_ptr=None, initial_ptr=None, stream=0):
        """raw pointers; initial_ptr: device array of n_channels doubles or None"""
        self.plan.launch(out_ptr, self.n if out_stride is None else out_stride, zi_ptr, zf_ptr, initial_ptr, stream)

    def launch_torch(self, out, initial=0.0, zi=None, zf=None):
        """out: (n_channels, >= n) row-contiguous device tensor of the plan dtype (rows may be windows of a wider
        tensor); `initial`: a scalar, one value per row, or a (n_channels,) float64 device tensor; zi / zf: optional
        (n_channels, state_dim) float64 device tensors.  Asynchronous on torch's current stream.  -> out"""
        import torch
        ptr, stride = _rows.check_rows(
            out, self.n_channels, self.n, _rows.torch_dtype(self.dtype),
            'out must be a (n_channels, >=n) row-contiguous device tensor of the plan dtype')
        zip_, zfp = _state_ptrs(zi, zf, self.n_channels, self.state_dim, 'n_channels')
        ini = _initial_rows(self, self.n_channels, initial, out.device)
        self.launch(ptr, stride, zip_, zfp, None if ini is None else ini.data_ptr(),
                    torch.cuda.current_stream(out.device).cuda_stream)
        return out

    def to_host(self, initial=0.0, zi=None, return_zf=False):
        """NumPy result (n_channels, n) [, zf (n_channels, state_dim)]; initial: a scalar or one value per row;
        zi: (n_channels, state_dim)"""
        return _host_trip(lambda out, reports, dzi, dzf, levels: self.launch(out, None, dzi, dzf, levels),
                          shape=(self.n_channels, self.n), dtype=self.dtype, rows=self.n_channels,
                          state_dim=self.state_dim, zi=zi, return_zf=return_zf, initial=initial)

    def close(self):
        self.plan.close()


def fir_host(sig: np.ndarray, ker: np.ndarray) -> np.ndarray:
    """NumPy in, NumPy out: upload, overlap-save FIR on the device, download.  Complex signals and / or
    kernels (the reference's `fftconvolve` takes both, distortion.py:329-337) run as real convolutions of
    their parts: (sr + i si) * (kr + i ki) = sr*kr - si*ki + i (sr*ki + si*kr)."""
    sig, ker = np.asarray(sig), np.asarray(ker)
    if np.iscomplexobj(sig) or np.iscomplexobj(ker):
        shape = np.shape(sig)
        rows = np.atleast_2d(sig)
        parts = [np.ascontiguousarray(rows.real, dtype=np.float64)]
        if np.iscomplexobj(sig):
            parts.append(np.ascontiguousarray(rows.imag, dtype=np.float64))
        stacked = np.concatenate(parts, axis=0)              # the parts as extra rows: one launch per kernel part
        nb = rows.shape[0]
        a = _fir_host_real(stacked, np.ascontiguousarray(ker.real, dtype=np.float64))
        out = a[:nb].astype(np.complex128)
        if len(parts) == 2:
            out += 1j * a[nb:]
        if np.iscomplexobj(ker):
            b = _fir_host_real(stacked, np.ascontiguousarray(ker.imag, dtype=np.float64))
            out += 1j * b[:nb]
            if len(parts) == 2:
                out -= b[nb:]
        return out.reshape(shape)
    return _fir_host_real(sig, ker)


def _fir_host_real(sig: np.ndarray, ker: np.ndarray) -> np.ndarray:
    sig2 = np.ascontiguousarray(np.atleast_2d(sig), dtype=np.float64)
    batch, n = sig2.shape
    if n == 0:
        return np.zeros_like(np.asarray(sig, dtype=np.float64))
    with _engine.FirPlan(ker, n, batch, np.float64) as plan, _engine.DeviceBuffer(sig2.nbytes) as din, \
            _engine.DeviceBuffer(sig2.nbytes) as dout:
        din.upload(sig2)
        plan.apply(din.ptr, n, dout.ptr, n)
        _engine.sync()
        return dout.download(sig2.shape, np.float64).reshape(np.shape(sig))


def combine_filters(filters):
    """Product of the (b, a) transfer functions (reference: distortion.py:226-244)."""
    b, a = np.poly1d([1.0]), np.poly1d([1.0])
    for b_, a_ in filters:
        b = b * np.poly1d(b_)
        a = a * np.poly1d(a_)
    return b.coeffs, a.coeffs


def exp_decay_filter(amp, tau, sample_rate, inv=False, output='ba'):
    """Multi-exponential step-response filter: u(t) -> u(t)(1 - sum A_i exp(-t/tau_i))
    (reference: distortion.py:100-185).  Returns (b, a), sos or (z, p, k)."""
    from scipy.signal import zpk2sos, zpk2tf
    if isinstance(amp, (int, float, complex)):
        amp, tau = [amp], [tau]
    num, den = np.poly1d([0.0]), np.poly1d([1.0])
    for i, (A, t) in enumerate(zip(amp, tau)):
        den = den * np.poly1d([1, -1 / t])
        term = np.poly1d([-A, 0.0])
        for j, t_ in enumerate(tau):
            if j != i:
                term = term * np.poly1d([1, -1 / t_])
        num = num + term
    num = num + den
    z = np.exp(-num.roots / sample_rate)
    p = np.exp(-1 / (np.asarray(tau) * sample_rate))
    if inv:
        z, p = p, z
    p = p[np.abs(p) < 1]
    k = (np.prod(1 - p) / np.prod(1 - z)).real
    if output == 'sos':
        return zpk2sos(z, p, k)
    if output == 'ba':
        return zpk2tf(z, p, k)
    if output == 'zpk':
        return z, p, k
    raise ValueError(f"Invalid output type: {output}")


def iir_host(sig, sections, zi=None, initial=0.0, ker=None):
    """NumPy in/out: upload, IIR scan (+ optional FIR) on the device, download.
    Returns (y, zf) with zf the final filter state (scipy layout).  A complex signal, initial value or
    state (scipy's lfilter / sosfilt take them; reference distortion.py:298-321) runs as two real passes:
    the coefficients are real, so real and imaginary parts filter independently."""
    cplx = np.iscomplexobj(sig) or np.iscomplexobj(initial) or (zi is not None and np.iscomplexobj(zi))
    if cplx or (ker is not None and np.iscomplexobj(ker)):
        if any(np.iscomplexobj(np.asarray(c)) for sec in sections for c in sec):
            raise NotImplementedError('IIR sections with complex coefficients')
        sig = np.asarray(sig)
        kr = None if (ker is None or np.iscomplexobj(ker)) else ker
        zr = None if zi is None else np.real(zi)
        yr, zfr = iir_host(np.real(sig), sections, zr, float(np.real(initial)), kr)
        if cplx:
            zim = None if zi is None else np.imag(zi)
            yi, zfi = iir_host(np.imag(sig), sections, zim, float(np.imag(initial)), kr)
            y, zf = yr + 1j * yi, zfr + 1j * zfi
        else:
            y, zf = yr, zfr
        if ker is not None and kr is None:
            y = fir_host(y, ker)
        return y, zf
    sig2 = np.ascontiguousarray(np.atleast_2d(sig), dtype=np.float64)
    batch, n = sig2.shape
    with contextlib.ExitStack() as stack:
        plan = stack.enter_context(_engine.IirPlan(sections, n, batch, np.float64))
        D = plan.state_dim
        x, y = _dev(stack, sig2.nbytes), _dev(stack, sig2.nbytes)
        x.upload(sig2)
        dzi = None
        if zi is not None:
            z = np.ascontiguousarray(np.broadcast_to(np.asarray(zi, dtype=np.float64).reshape(-1),
                                                     (batch, D)))
            dzi = _dev(stack, z.nbytes)
            dzi.upload(z)
        dzf = _dev(stack, batch * D * 8)
        if not _engine.iir_run_checked(      # (x stays intact: a launch whose look-back timed out can be repeated)
                lambda: plan.apply(x.ptr, n, y.ptr, n, dzi.ptr if dzi else None, dzf.ptr, initial), plan.status):
            raise _engine.EngineError('IIR stage failed twice')
        res = y
        if ker is not None and n > 0:
            stack.enter_context(_engine.FirPlan(ker, n, batch, np.float64)).apply(y.ptr, n, x.ptr, n)
            res = x
        _engine.sync()
        out = res.download(sig2.shape, np.float64) if n else sig2.copy()
        zf = dzf.download((batch, D), np.float64) if n else np.zeros((batch, D))
    return out.reshape(np.shape(sig)), (zf[0] if np.ndim(sig) == 1 else zf)


class CascadeState(np.ndarray):
    """The `zf` that `predistort(..., return_zf=True)` hands out for a combined filter order > 16: the
    direct-form-II-transposed states of the caller's sections back to back (NOT scipy.signal.lfilter's state
    of the combined polynomials, which has the same length).  Only such an array is accepted back as `zi`
    on that path, so an lfilter-format state cannot be misread silently."""


def predistort(sig, filters=None, ker=None, initial=0.0, initial_x=None,
               initial_y=None, zi=None, return_zf=False):
    """reference: waveforms/distortion.py:289-337, both branches on the GPU.

    Combined filter order <= 16 (every exp-decay correction with up to 16 time constants): the reference's
    semantics to the letter -- `zi` / the returned `zf` are scipy.signal.lfilter's state of the combined
    (b, a), `initial` / `initial_x` / `initial_y` seed it through lfiltic.

    Combined order > 16: a direct form of that order is not usable in double precision (the reference's own
    lfilter returns 1e125 / NaN once poles crowd z = 1), so the caller's sections run as a cascade:
      * `initial=c` starts every section in its steady state for the level that reaches it (c times the DC
        gains before it).  For sections of unit DC gain -- every exp_decay_filter -- this IS the reference's
        `initial_x = initial_y = c`; tests/golden/iir.npz holds reference runs of order 17 and 20 where its
        direct form is still accurate, and the cascade agrees with them to 1e-9.
      * `return_zf` hands out a `CascadeState`; `zi` must be one (ValueError otherwise).
      * `initial_x` / `initial_y` histories cannot be expressed: ValueError."""
    sig = np.asarray(sig)
    zf = None
    if filters is not None:
        from scipy.signal import lfiltic, tf2zpk
        b, a = combine_filters(filters)
        _, p, _ = tf2zpk(b, a)
        if not np.all(np.abs(p) < 1):
            warnings.warn('Warning: filter is unstable')
        if max(len(b), len(a)) - 1 > 16:
            if initial_x is not None or initial_y is not None:
                raise ValueError('predistort: a combined filter of order > 16 has no usable direct form in double '
                                 'precision; initial_x / initial_y histories cannot be honoured -- use initial=')
            if zi is not None and not isinstance(zi, CascadeState):
                raise ValueError('predistort: for a combined filter order > 16 `zi` must be the CascadeState that '
                                 'return_zf=True handed out (the sections\' states back to back); an lfilter-format '
                                 'state of the combined polynomials has the same length but another meaning')
            return _predistort_high_order(sig, filters, zi, ker, return_zf, complex(initial) if zi is None else None)
        if zi is None:
            ix = (np.full((len(b) - 1, ), initial) if initial_x is None else
                  np.asarray(initial_x)[:len(b) - 1])
            iy = (np.full((len(a) - 1, ), initial) if initial_y is None else
                  np.asarray(initial_y)[:len(a) - 1])
            zi = lfiltic(b, a, iy, ix)
        sections = [(b, a)]
        sig, zf = iir_host(sig, sections, zi=zi, ker=ker)
        return (sig, zf) if return_zf else sig
    if ker is None:
        return (sig, zf) if return_zf else sig
    out = fir_host(sig, np.asarray(ker))
    return (out, zf) if return_zf else out


def _predistort_high_order(sig, filters, zi, ker, return_zf, steady):
    """predistort(filters=...) for a combined order > 16 (reference distortion.py:298-321: one lfilter call on
    the product polynomials), which has no single device section -- and no usable direct form at all: with
    twenty poles next to z = 1 the free response of a direct-form state is the difference of terms 1e50
    times its size, the reference's own double-precision lfilter returns 1e125 or NaN on such sections
    (measured; tests/test_gpu_iir.py), and a state vector of doubles cannot even carry the information.
    The same LTI system is the cascade of the caller's own sections, run on the device:
      * `initial=c` ("the line sat at c for ever", steady != None): every section starts in ITS steady state
        for the constant level that reaches it, c times the DC gains before it -- exact, well conditioned;
      * zi / return_zf: the state is the CASCADE's (the sections' direct-form-II-transposed states back to
        back, sum of the section orders = the combined order values): what `return_zf` hands out, `zi`
        takes back, and a signal processed in pieces equals the signal processed whole."""
    secs = [(np.atleast_1d(np.asarray(b_, dtype=np.float64)), np.atleast_1d(np.asarray(a_, dtype=np.float64)))
            for b_, a_ in filters]
    orders = [max(len(b_), len(a_)) - 1 for b_, a_ in secs]
    zsec = None
    if steady is not None:
        if steady != 0:
            # (a complex level -- scipy takes a complex `initial` -- seeds real and imaginary parts alike:
            #  the sections are real and lfiltic is linear in its histories)
            from scipy.signal import lfiltic
            level, parts = (steady if steady.imag != 0 else steady.real), []
            for (b_, a_), m in zip(secs, orders):
                gain = b_.sum() / a_.sum()
                z = lfiltic(b_, a_, np.full(len(a_) - 1, level * gain), np.full(len(b_) - 1, level))
                parts.append(np.concatenate([z, np.zeros(m - len(z))]))
                level *= gain
            zsec = np.concatenate(parts)
    elif zi is not None:
        zsec = np.asarray(zi).reshape(-1)
        if len(zsec) != sum(orders):
            raise ValueError(f'predistort: zi must hold the {sum(orders)} cascade state values')
    out, zf = iir_host(sig, secs, zi=zsec, ker=ker)
    return (out, np.asarray(zf).view(CascadeState)) if return_zf else out


def distort(points, params, sample_rate, initial=0.0):
    """reference: waveforms/distortion.py:340-346."""
    filters = []
    for amp, tau in np.asarray(params).reshape(-1, 2):
        filters.append(exp_decay_filter(amp, abs(tau), sample_rate))
    return predistort(points, filters, initial=initial)


ROWS_MAX_ORDER = 4     # combined order per row that the per-row plan takes (state dimension <= 4)


def _rows_arguments(sig, filters_rows, initial, zi):
    """host-side checks and filter design of predistort_rows: -> (sig, [(b, a)] per row, initial (batch,), zi or None)"""
    sig = np.asarray(sig)
    if sig.ndim != 2:
        raise ValueError('predistort_rows: sig must be 2-D (rows, samples)')
    batch = sig.shape[0]
    filters_rows = list(filters_rows)
    if len(filters_rows) != batch:
        raise ValueError(f'predistort_rows: {len(filters_rows)} filter lists for {batch} rows')
    ini = np.asarray(initial)
    if ini.ndim == 0:
        ini = np.full(batch, ini[()])
    if ini.shape != (batch, ):
        raise ValueError('predistort_rows: initial is a scalar or one value per row')
    ba = []
    for filters in filters_rows:
        filters = list(filters)
        if any(np.iscomplexobj(np.asarray(c)) for sec in filters for c in sec):
            raise NotImplementedError('IIR sections with complex coefficients')
        b, a = combine_filters(filters)
        ba.append((np.atleast_1d(np.asarray(b, dtype=np.float64)), np.atleast_1d(np.asarray(a, dtype=np.float64))))
    if zi is not None:
        zi = [np.atleast_1d(np.asarray(z)) for z in zi]
        if len(zi) != batch:
            raise ValueError(f'predistort_rows: {len(zi)} states for {batch} rows')
        for r, ((b, a), z) in enumerate(zip(ba, zi)):
            if z.shape != (max(len(b), len(a)) - 1, ):
                raise ValueError(f'predistort_rows: zi[{r}] must hold the {max(len(b), len(a)) - 1} lfilter state '
                                 f'values of row {r}')
    return sig, ba, ini, zi


def _iir_rows_real(sig2, ba, zi):
    """real rows through one IirRowsPlan launch: -> (out, [zf per row]); ba: one combined (b, a) per row"""
    batch, n = sig2.shape
    sig2 = np.ascontiguousarray(sig2, dtype=np.float64)
    with contextlib.ExitStack() as stack:
        plan = stack.enter_context(_engine.IirRowsPlan([[s] for s in ba], n, np.float64))
        z = np.zeros((batch, plan.state_dim))
        for r, zr in enumerate(zi):
            z[r, :len(zr)] = zr
        x, dzi, dzf = _dev(stack, sig2.nbytes), _dev(stack, z.nbytes), _dev(stack, z.nbytes)
        x.upload(sig2)
        dzi.upload(z)
        plan.apply(x.ptr, n, x.ptr, n, dzi.ptr, dzf.ptr)
        _engine.sync()
        out = x.download(sig2.shape, np.float64)
        zf = dzf.download(z.shape, np.float64)
    return out, [zf[r, :plan.own_orders[r][0]] for r in range(batch)]


def predistort_rows(sig, filters_rows, initial=0.0, zi=None, return_zf=False):
    """`predistort(sig[r], filters_rows[r], initial=initial[r])` for every row r of a 2-D `sig` (reference
    distortion.py:298-321 per row: one lfilter over the row's combined (b, a), started from lfiltic for the level
    `initial[r]`), all rows in ONE launch with one filter per row.

    filters_rows: one list of (b, a) sections per row.  initial: a scalar or one value per row.  zi: optional, one
    lfilter state per row (row r: combined order of that row), used instead of lfiltic.  return_zf: also return the
    list of final states, one array per row (rows differ in length when their orders do).
    Complex rows / levels / states run as two real passes.  A row whose poles are not all inside the unit circle
    warns 'filter is unstable' as predistort does.
    Rows whose combined order exceeds 4 do not fit the per-row plan: they go through `predistort` one by one
    (correct, one launch per row -- slow).
    Raises ValueError (sig not 2-D, wrong number of rows, initial neither scalar nor one value per row, a zi of
    the wrong length) and NotImplementedError (complex coefficients) before any device work."""
    from scipy.signal import lfiltic, tf2zpk
    sig, ba, ini, zi = _rows_arguments(sig, filters_rows, initial, zi)
    batch, n = sig.shape
    unstable = False
    for b, a in ba:
        _, p, _ = tf2zpk(b, a)
        unstable = unstable or not np.all(np.abs(p) < 1)
    if unstable:
        warnings.warn('Warning: filter is unstable')
    if zi is None:
        zi = [lfiltic(b, a, np.full(len(a) - 1, c), np.full(len(b) - 1, c)) for (b, a), c in zip(ba, ini)]
    cplx = np.iscomplexobj(sig) or any(np.iscomplexobj(z) for z in zi)
    out = np.empty(sig.shape, dtype=np.complex128 if cplx else np.float64)
    zf = [None] * batch
    small = [r for r, (b, a) in enumerate(ba) if max(len(b), len(a)) - 1 <= ROWS_MAX_ORDER]
    big = [r for r in range(batch) if max(len(ba[r][0]), len(ba[r][1])) - 1 > ROWS_MAX_ORDER]
    if n == 0:
        out[...] = sig
        zf = [np.array(z) for z in zi]
    else:
        if small:
            sub = [ba[r] for r in small]
            o, z = _iir_rows_real(np.real(sig[small]), sub, [np.real(zi[r]) for r in small])
            if cplx:
                oi, zim = _iir_rows_real(np.imag(sig[small]), sub, [np.imag(zi[r]) for r in small])
                o, z = o + 1j * oi, [p + 1j * q for p, q in zip(z, zim)]
            out[small] = o
            for r, zr in zip(small, z):
                zf[r] = zr
        for r in big:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')            # (warned once above)
                o, z = predistort(sig[r], [ba[r]], zi=zi[r], return_zf=True)
            out[r], zf[r] = o, (z + 0j if cplx else z)
    return (out, zf) if return_zf else out


def distort_rows(points, params_rows, sample_rate, initial=0.0):
    """`distort(points[r], params_rows[r], sample_rate, initial[r])` for every row of a 2-D `points` (reference
    distortion.py:340-346 per row): params_rows[r] = [amp0, tau0, amp1, tau1, ...] of line r; rows may have
    different numbers of time constants.  One launch (see predistort_rows, whose errors it shares)."""
    points = np.asarray(points)
    params_rows = list(params_rows)
    if points.ndim != 2 or len(params_rows) != points.shape[0]:
        raise ValueError('distort_rows: points must be 2-D with one parameter list per row')
    filters_rows = [[exp_decay_filter(amp, abs(tau), sample_rate) for amp, tau in np.asarray(p).reshape(-1, 2)]
                    for p in params_rows]
    return predistort_rows(points, filters_rows, initial=initial)


# --------------------------------------------------------------------------
# the Z-distortion fit model (reference distortion.py:349-366)
# --------------------------------------------------------------------------
def _phase_geometry(t, pulse_width, start, sample_rate):
    """host side of phase_curve, before any device work: -> (t as float64 array, lim, num, pp, sp).
    ValueError wherever the reference raises: an empty t (np.max of nothing), a NaN t (round(nan)), a negative
    sp (np.zeros of a negative length), an empty kernel (np.convolve: v cannot be empty) and a kernel longer
    than the signal (np.convolve then returns pp + sp values, which np.interp refuses next to num grid values)."""
    tq = np.asarray(t, dtype=np.float64)
    if tq.size == 0:
        raise ValueError('phase_curve: t is empty')
    lim = max(np.max(np.abs(tq)), 20e-6)
    num = round(2 * lim * sample_rate)                     # (ValueError for a NaN)
    pp = round(pulse_width * sample_rate)
    sp = round((start + pulse_width) * sample_rate) - 1
    if pp < 0 or sp < 0:
        raise ValueError(f'phase_curve: negative kernel dimensions (pulse points {pp}, start points {sp})')
    if pp + sp == 0:
        raise ValueError('phase_curve: the kernel is empty (pulse points + start points == 0)')
    if pp + sp > num:
        raise ValueError(f'phase_curve: the kernel ({pp + sp} points) is longer than the signal ({num} points)')
    return tq, lim, num, pp, sp


def _param_rows(params_rows):
    rows = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in params_rows]
    if not rows:
        raise ValueError('no parameter rows')
    return rows


class PhaseCurve:
    """`phase_curve(t, params, df_dphi, pulse_width, start, wav, sample_rate)` (reference distortion.py:349-366)
    for MANY parameter sets, built once per fit: the wave is sampled once (`wav(tlist)`, the drop-in call) and its
    row stays on the device, the probe plan (csrc/wfk_probe.hip) is built once; an evaluation of P parameter sets is
    ONE per-row IIR launch that reads that row P times (`IirRowsPlan.apply_shared_in`) plus ONE probe launch, both
    asynchronous on torch's current stream.

        pc = PhaseCurve(x, df_dphi, 10e-9, 25e-9, wav, 2e9)
        popt, pcov = curve_fit(pc.model, x, y, p0=[-0.03, 0.1e-6, 0.02, 0.3e-6], jac=pc.jac_model)

    pc(params) -> (nq,); pc.rows(params_rows) -> (P, nq) NumPy; pc.rows_torch(params_rows, out=None) -> device
    tensor; pc.jac(params) -> (nq, len(params)), forward differences, p and every p + h e_k rows of one evaluation.
    Row r's params are [amp0, tau0, amp1, tau1, ...] with any number of time constants (rows may differ); its filter is
    the CASCADE of the first-order sections exp_decay_filter(amp, |tau|, sample_rate), from rest -- in exact arithmetic
    the reference's combined (b, a), numerically better conditioned.  A launch takes four
    sections per row: rows with more than 4 constants cost one more in-place IIR launch over the workspace per further
    four constants -- correct, but slower than the one-launch shape of a usual fit.  The (P, num) workspace is kept and
    grown as needed."""

    def __init__(self, t, df_dphi, pulse_width, start, wav, sample_rate):
        self.t, lim, self.num, self.pp, self.sp = _phase_geometry(t, pulse_width, start, sample_rate)
        self.shape = self.t.shape
        self.sample_rate = sample_rate
        self.nq = self.t.size
        self.tlist = np.arange(self.num) / sample_rate - lim
        self._x_host = np.ascontiguousarray(wav(self.tlist), dtype=np.float64)
        if self._x_host.shape != (self.num, ):
            raise ValueError('phase_curve: wav(tlist) must give one real sample per time')
        import torch
        self._dev = torch.device('cuda', torch.cuda.current_device())
        self._x = torch.from_numpy(self._x_host).to(self._dev)
        self.gain = 2 * np.pi * df_dphi / sample_rate
        self.probe = _engine.BoxProbePlan(self.tlist, self.t.reshape(-1), self.pp, (self.pp + self.sp - 1) // 2,
                                          self.gain)
        self._ws = None
        self._iir = []            # the plans of the last evaluation: their tables live until the next one replaces them

    def sections(self, params):
        """[[(b, a)] * 4, ...]: the first-order sections exp_decay_filter(amp, |tau|, sample_rate) of one parameter set
        in groups of four (one group per IIR launch), the last group filled up with pass-through sections; no time
        constant at all: one group of pass-through sections.  EVERY row runs in the four-section shape, whatever
        else is in its batch: a row's result is then bitwise the same in any batch and on its own."""
        secs = [exp_decay_filter(amp, abs(tau), self.sample_rate)
                for amp, tau in np.asarray(params, dtype=np.float64).reshape(-1, 2)]
        secs += [([1.0, 0.0], [1.0, 0.0])] * (-len(secs) % ROWS_MAX_ORDER or (0 if secs else ROWS_MAX_ORDER))
        return [secs[i:i + ROWS_MAX_ORDER] for i in range(0, len(secs), ROWS_MAX_ORDER)]

    def rows_torch(self, params_rows, out=None):
        """-> (P, nq) float64 device tensor (`out`, row-contiguous, when given); asynchronous on the current stream"""
        import torch
        rows = _param_rows(params_rows)
        P = len(rows)
        if out is None:
            out = torch.empty((P, self.nq), dtype=torch.float64, device=self._dev)
        out_ptr, out_stride = _rows.check_rows(
            out, P, self.nq, torch.float64, f'out must be a ({P}, {self.nq}) row-contiguous float64 device tensor',
            exact=True)
        if self._ws is None or self._ws.shape[0] < P:
            self._ws = None
            self._ws = torch.empty((P, self.num), dtype=torch.float64, device=self._dev)
        ws = self._ws
        stream = torch.cuda.current_stream(self._dev).cuda_stream
        groups = [self.sections(p) for p in rows]
        for plan in self._iir:                # (the tables of the last evaluation lived until here)
            plan.close()
        self._iir = []
        passthrough = [([1.0, 0.0], [1.0, 0.0])] * ROWS_MAX_ORDER
        for k in range(max(len(g) for g in groups)):
            # pass k: the k-th group of four sections of every row that has one.  Pass 0 reads the one sampled row;
            # later passes (rows with more than 4 constants) filter the workspace in place, over the span of rows
            # that need them -- rows in between without a k-th group take pass-through sections, which are exact.
            need = [r for r in range(P) if len(groups[r]) > k]
            lo, hi = (0, P) if k == 0 else (need[0], need[-1] + 1)
            plan = _engine.IirRowsPlan([groups[r][k] if len(groups[r]) > k else passthrough for r in range(lo, hi)],
                                       self.num, np.float64)
            self._iir.append(plan)
            if k == 0:
                plan.apply_shared_in(self._x.data_ptr(), ws.data_ptr(), ws.stride(0), stream=stream)
            else:
                at = ws[lo].data_ptr()
                plan.apply(at, ws.stride(0), at, ws.stride(0), stream=stream)
        self.probe.apply(ws.data_ptr(), P, ws.stride(0), out_ptr, out_stride, stream)
        return out

    def rows(self, params_rows):
        """-> (P, nq) NumPy array"""
        return self.rows_torch(params_rows).cpu().numpy()

    def __call__(self, params):
        """-> what the reference's phase_curve returns for `params`: np.interp's shape and dtype for `t`"""
        return self.rows([params])[0].reshape(self.shape)[()]

    @staticmethod
    def step(params, rel_step=None):
        """the forward-difference steps of scipy.optimize.curve_fit's default method ('lm': MINPACK's fdjac2):
        h_k = rel_step * |p_k|, rel_step = sqrt(machine epsilon) when None, and h_k = rel_step where p_k == 0"""
        p = np.asarray(params, dtype=np.float64).reshape(-1)
        rel = np.sqrt(np.finfo(np.float64).eps) if rel_step is None else float(rel_step)
        h = rel * np.abs(p)
        return np.where(h == 0, rel, h)

    def jac(self, params, rel_step=None):
        """-> (nq, len(params)): column k is (f(p + h_k e_k) - f(p)) / h_k with `step`'s h; ONE evaluation of
        1 + len(params) rows"""
        p = np.asarray(params, dtype=np.float64).reshape(-1)
        h = self.step(p, rel_step)
        f = self.rows([p] + [np.where(np.arange(len(p)) == k, p + h, p) for k in range(len(p))])
        return ((f[1:] - f[0]) / h[:, None]).T

    def model(self, t_ignored, *params):
        """f of `curve_fit(f, x, y, p0)`: the probe times are those of the constructor"""
        return np.asarray(self(params)).reshape(-1)

    def jac_model(self, t_ignored, *params):
        """jac of `curve_fit(f, x, y, p0, jac=)`"""
        return self.jac(params)

    def close(self):
        self.probe.close()
        for plan in self._iir:
            plan.close()
        self._iir = []
        self._ws = self._x = None


def phase_curve(t, params, df_dphi, pulse_width, start, wav, sample_rate):
    """reference: waveforms/distortion.py:349-366 -- the phase a qubit picks up from a Z pulse `wav` distorted by the
    exp-decay `params`, integrated over `pulse_width` and read off at the delays `t`.  Same signature, same return
    (np.interp's shape and dtype, a scalar t included), ValueError wherever the reference raises.  One `PhaseCurve`
    evaluation; a fit should build a `PhaseCurve` once instead."""
    with contextlib.closing(PhaseCurve(t, df_dphi, pulse_width, start, wav, sample_rate)) as pc:
        return pc(params)


# --------------------------------------------------------------------------
# FFT-domain operations
# --------------------------------------------------------------------------
def reflection_filter(f, A, tau):
    """Transfer function of a single reflection (reference: distortion.py:188-205)."""
    return (1 - A) / (1 - A * np.exp(-2j * np.pi * f * tau))


def transfer_host(sig, H):
    """irfft(rfft(sig) * H) on the device; H: the n//2+1 non-negative-frequency bins."""
    sig = np.ascontiguousarray(sig, dtype=np.float64)
    n = len(sig)
    Hc = np.ascontiguousarray(H, dtype=np.complex128)
    assert Hc.shape == (n // 2 + 1, )
    with _engine.SpectralPlan(n, 1, np.float64) as plan, _engine.DeviceBuffer(n * 8) as x, \
            _engine.DeviceBuffer(n * 8) as y, _engine.DeviceBuffer(Hc.nbytes) as h:
        x.upload(sig)
        h.upload(Hc)
        plan.apply(x.ptr, y.ptr, h.ptr)
        _engine.sync()
        return y.download((n, ), np.float64)


def reflection(sig, A, tau, sample_rate):
    """ifft(fft(sig) * H(f)).real with H the reflection filter
    (reference: distortion.py:208-210); whole-signal FFT on the device."""
    freq = np.fft.rfftfreq(len(sig), 1 / sample_rate)
    return transfer_host(sig, reflection_filter(freq, A, tau))


def correct_reflection(sig, A, tau, sample_rate=None):
    """Inverse of `reflection` (reference: distortion.py:213-223); symbolic for a Waveform."""
    from .waveform import Waveform
    if isinstance(sig, Waveform):
        return 1 / (1 - A) * sig - A / (1 - A) * (sig >> tau)
    if sample_rate is None:
        raise ValueError('sample_rate is not given')
    freq = np.fft.rfftfreq(len(sig), 1 / sample_rate)
    return transfer_host(sig, 1 / reflection_filter(freq, A, tau))


def shift(signal, delay, dt):
    """Delay a sampled signal by `delay` (3-tap fractional interpolation on the device +
    integer shift; reference: distortion.py:12-39)."""
    signal = np.asarray(signal)          # (dtype kept as upstream does: complex signals stay complex)
    points = int(delay // dt)
    delta = delay / dt - points
    if delta > 0:
        signal = fir_host(signal, np.array([0, 1 - delta, delta]))
    if points == 0:
        return signal
    ret = np.zeros_like(signal)
    if points < 0:
        ret[:points] = signal[-points:]
    else:
        ret[points:] = signal[:-points]
    return ret


class ReflectionStage:
    """Device-resident reflection / delay stage for `len(terms_rows)` rows of `n` samples (build once, apply many
    times), the counterpart of `IirStage` rows for the FFT-domain part of a line's calibration:
        y[r] = ifft(fft(x[r]) * H_r(f)).real,   H_r = the product of row r's terms
    with `reflection_filter(f, A, tau)` for ('reflect', A, tau), its inverse for ('correct', A, tau) -- what
    `reflection` / `correct_reflection` apply to one signal -- and exp(-2j pi f tau) for ('delay', tau), tau of either
    sign.  A row may carry up to `_engine.SPEC_ROWS_MAX_TERMS` terms (ValueError beyond), or none (it passes unchanged);
    |A| >= 1 is refused (the reference's filter divides by zero at A = 1).  One transform pair per apply whatever the
    number of terms; the transfer functions are formed on the device, nothing but the small term table is uploaded.

        st = ReflectionStage([[('correct', A, tau), ('delay', -skew)] for A, tau, skew in lines], n, 2e9)
        st.apply_torch(x)                      # in place, on torch's current stream
        st.apply_torch(x, out=y)
    """

    def __init__(self, terms_rows, n: int, sample_rate: float, dtype=np.float64):
        self.plan = _engine.SpectralRowsPlan(terms_rows, n, sample_rate, dtype)
        self.n, self.batch, self.dtype = self.plan.n, self.plan.batch, self.plan.dtype
        self.sample_rate = self.plan.sample_rate

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, stream=0):
        self.plan.apply(in_ptr, in_stride, out_ptr, out_stride, stream)

    def apply_torch(self, x, out=None):
        """x, out: (batch, >= n) row-contiguous device tensors of the stage's dtype (rows may be windows of a wider
        tensor, any row stride >= n); out=None or out is x: in place.  Asynchronous on torch's current stream; one
        stage serves one stream at a time (it owns the transform buffers).  -> out"""
        import torch
        out = x if out is None else out
        (x0, xs), (y0, ys) = (_rows.check_rows(
            t, self.batch, self.n, _rows.torch_dtype(self.dtype),
            'expected (batch, >=n) row-contiguous device tensors of the stage dtype') for t in (x, out))
        self.apply(x0, xs, y0, ys, torch.cuda.current_stream(x.device).cuda_stream)
        return out

    def close(self):
        self.plan.close()


def _per_row(name, what, value, batch):
    """a scalar (every row) or one entry per row -> list of `batch` entries"""
    if not isinstance(value, (list, tuple, np.ndarray)) or (isinstance(value, np.ndarray) and value.ndim == 0):
        return [value] * batch
    value = list(value)
    if len(value) != batch:
        raise ValueError(f'{name}: {len(value)} {what} entries for {batch} rows')
    return value


def _per_row_flat(name, what, v, batch):
    """`_per_row` for a stage's numbers: an array of any shape counts as its entries in order, a 0-d one as a scalar"""
    return _per_row(name, what, list(np.asarray(v).reshape(-1)) if np.ndim(v) > 0 else v, batch)


def _gain_offset_rows(who, gain, offset, rows):
    """the converter's per-row arguments: each a scalar (every row) or one value per row -> (gains, offsets), lists"""
    return _per_row_flat(who, 'gain', gain, rows), _per_row_flat(who, 'offset', offset, rows)


def _given_rows(gain, offset):
    """the number of rows that a gain or an offset given per row speaks of; 1 where both are scalars"""
    return max(np.size(gain) if np.ndim(gain) > 0 else 1, np.size(offset) if np.ndim(offset) > 0 else 1)


def _full_scale_gain(who, full_scale, kw):
    """the gain of a `from_full_scale`, hi / full scale, with `bits` as the constructor's keywords `kw` have it (16
    without); ValueError: bits outside [2, 16], a full scale that is not finite or not positive"""
    bits = int(kw.get('bits', 16))
    if not 2 <= bits <= 16:
        raise ValueError('bits must lie in [2, 16]')
    fs = np.asarray(full_scale, dtype=np.float64)
    if not np.all(np.isfinite(fs) & (fs > 0.0)):
        raise ValueError(f'{who}: every full scale must be finite and positive')
    return (2**(bits - 1) - 1) / fs


def _check_reports(stage, name, rows_name, rows, sides, counts=None, beyond=None, zi=None, zf=None, state_dim=0):
    """What goes with the int16 codes of an `apply_torch` / `launch_torch`, once x and the codes have passed
    `_rows.check_rows` in that order: `sides` are the two, (x, codes) or (codes, ) for a sampled chain, as
    `_rows.rows_disjoint` takes them.  counts / beyond: None or contiguous (rows, 3) int64 device tensors; zi / zf: None
    or (rows, state_dim) float64.  Tensor metadata only, texts ready made: nothing is built, formatted or read from
    the device unless a refusal is raised, and those come in ONE order: counts, beyond, zi / zf, the codes over x,
    counts over x / codes, beyond over x / codes, beyond over counts.  `stage`: the short name the overlap texts
    begin with; `name`: what they call the codes; `rows_name`: what the other texts call the rows.
    -> (counts pointer, beyond pointer, zi pointer, zf pointer), None for what is not there"""
    counts_text, beyond_text, _ = _FRONT_TEXTS[rows_name]
    c0 = _rows.check_state(counts, (rows, 3), counts_text, dtype=np.int64)
    b0 = _rows.check_state(beyond, (rows, 3), beyond_text, dtype=np.int64)
    zip_, zfp = _state_ptrs(zi, zf, rows, state_dim, rows_name)
    if len(sides) == 2 and not _rows.rows_disjoint(*sides):
        raise ValueError(f'{stage} is out of place: {name} overlaps x')
    if not _rows.report_disjoint(c0, rows, 3, *sides):
        raise ValueError(f'{stage}: counts overlaps {"x / " * (len(sides) == 2)}{name}')
    if b0 is not None:
        if not _rows.report_disjoint(b0, rows, 3, *sides):
            raise ValueError(f'{stage}: beyond overlaps {"x / " * (len(sides) == 2)}{name}')
        if c0 is not None and not _rows.report_disjoint(b0, rows, 3, (c0, 3, rows, 3, 8)):
            raise ValueError(f'{stage}: beyond overlaps counts')
    return c0, b0, zip_, zfp


class _LentScratch:
    """For the sampled chains whose unfused path runs through float64 rows (`fused`, `n_channels`, `n`, `plan`): the
    rows are taken once, by the constructor, lent to every launch, and freed with the plan."""

    def _take_scratch(self):
        self._scratch = None if self.fused else _engine.DeviceBuffer(max(self.n_channels * self.n, 1) * 8)

    def close(self):
        self.plan.close()
        if self._scratch is not None:
            self._scratch.close()
            self._scratch = None


def _one_shot(sig2, plan, apply, shape, dtype, report_rows, reports, return_counts, initial=None):
    """The round trip of a NumPy one-shot wrapper whose arguments have passed: `plan()` opens the plan, the rows
    `sig2` go up, `apply(plan, x, y, [report pointers], levels)` launches on pointers -- y the result of `shape` and
    `dtype` (None: in place, y is x), the report pointers those of `reports` (report_rows, 3) int64 reports (None
    each unless `return_counts`), levels the (rows,) float64 `initial` or None where all are zero -- then one
    synchronise and the downloads.  Rows of no samples are answered with zeros, without a device.
    -> the result, or (result, the reports in order) with `return_counts`"""
    in_place = shape is None
    if in_place:
        shape, dtype = sig2.shape, sig2.dtype
    if sig2.shape[1] == 0:
        out = [np.zeros(shape, dtype=dtype)] + [np.zeros((report_rows, 3), dtype=np.int64) for _ in range(reports)]
        return tuple(out) if return_counts else out[0]
    with contextlib.ExitStack() as stack:
        plan = stack.enter_context(plan())
        x = _dev(stack, sig2.nbytes)
        y = x if in_place else _dev(stack, shape[0] * shape[1] * np.dtype(dtype).itemsize)
        rep = [_dev(stack, report_rows * 24) for _ in range(reports if return_counts else 0)]
        x.upload(sig2)
        levels = None
        if initial is not None and initial.any():
            lv = _dev(stack, initial.nbytes)
            lv.upload(np.ascontiguousarray(initial))
            levels = lv.ptr
        apply(plan, x.ptr, y.ptr, [r.ptr for r in rep] or [None] * reports, levels)
        _engine.sync()
        out = [y.download(shape, dtype)] + [r.download((report_rows, 3), np.int64) for r in rep]
        return tuple(out) if return_counts else out[0]


def _reflection_rows_terms(name, kind, batch, A_rows, tau_rows):
    """term lists of reflection_rows / correct_reflection_rows: A and tau each a scalar, or one entry per row, an entry
    a scalar or a sequence (several reflections on that row); within a row a scalar goes with every entry of the
    other's sequence"""
    rows = []
    for r, (A, tau) in enumerate(zip(_per_row(name, 'A', A_rows, batch), _per_row(name, 'tau', tau_rows, batch))):
        A, tau = np.atleast_1d(np.asarray(A, dtype=np.float64)), np.atleast_1d(np.asarray(tau, dtype=np.float64))
        if A.ndim != 1 or tau.ndim != 1 or (len(A) != len(tau) and 1 not in (len(A), len(tau))):
            raise ValueError(f'{name}: row {r} has {len(A)} amplitudes and {len(tau)} delays')
        A, tau = np.broadcast_arrays(A, tau)
        rows.append([(kind, float(a), float(t)) for a, t in zip(A, tau)])
    return rows


def _delay_rows_terms(batch, delays):
    return [[('delay', float(d))] for d in _per_row('delay_rows', 'delay', delays, batch)]


def _rows_signal(name, sig):
    sig = np.asarray(sig)
    if sig.ndim != 2:
        raise ValueError(f'{name}: sig must be 2-D (rows, samples)')
    if np.iscomplexobj(sig):
        raise NotImplementedError(f'{name}: complex rows')
    return np.ascontiguousarray(sig, dtype=np.float64)


def _rows_signal_f32(name, sig):
    """_rows_signal, but float32 rows stay float32"""
    src = np.asarray(sig)
    if src.ndim == 2 and src.dtype == np.float32:
        return np.ascontiguousarray(src)
    return _rows_signal(name, sig)


def _spectral_rows_host(sig2, terms_rows, sample_rate):
    """NumPy in, NumPy out: upload, one SpectralRowsPlan apply in place, download"""
    batch, n = sig2.shape
    if n == 0:
        _engine.pack_spec_terms(terms_rows)
        return sig2.copy()
    with _engine.SpectralRowsPlan(terms_rows, n, sample_rate, np.float64) as plan, \
            _engine.DeviceBuffer(sig2.nbytes) as x:
        x.upload(sig2)
        plan.apply(x.ptr, n, x.ptr, n)
        _engine.sync()
        return x.download(sig2.shape, np.float64)


def reflection_rows(sig, A_rows, tau_rows, sample_rate):
    """`reflection(sig[r], A_rows[r], tau_rows[r], sample_rate)` for every row r of a 2-D `sig` (reference
    distortion.py:208-210 per row), all rows in one launch, the transfer functions formed on the device.
    A_rows / tau_rows: a scalar (every row), or one entry per row; an entry may be a sequence: several reflections on
    that line, their filters multiplied (at most `_engine.SPEC_ROWS_MAX_TERMS`).  ValueError before any device work:
    sig not 2-D, a row count that does not match, amplitudes and delays of different lengths, |A| >= 1."""
    sig2 = _rows_signal('reflection_rows', sig)
    return _spectral_rows_host(
        sig2, _reflection_rows_terms('reflection_rows', 'reflect', sig2.shape[0], A_rows, tau_rows), sample_rate)


def correct_reflection_rows(sig, A_rows, tau_rows, sample_rate):
    """`correct_reflection(sig[r], A_rows[r], tau_rows[r], sample_rate)` for every row of a 2-D `sig` (reference
    distortion.py:213-223 per row); arguments and errors as `reflection_rows`, whose inverse it is."""
    sig2 = _rows_signal('correct_reflection_rows', sig)
    return _spectral_rows_host(
        sig2, _reflection_rows_terms('correct_reflection_rows', 'correct', sig2.shape[0], A_rows, tau_rows),
        sample_rate)


def delay_rows(sig, delays, sample_rate):
    """Row r of a 2-D `sig` delayed by `delays[r]` seconds (a scalar: every row; negative: advanced):
    ifft(fft(sig[r]) * exp(-2j pi f delays[r])).real -- the BAND-LIMITED, CIRCULAR delay: what leaves at one end of the
    row comes back in at the other, a whole number of samples is an exact np.roll, a fraction of a sample is the
    sinc interpolation of the periodic signal.  This is NOT `shift`, which follows the reference's 3-tap linear
    interpolation and fills with zeros; use `shift_rows` / `ShiftStage` for the reference's results on rows, this for
    skew correction of rows that are zero (or periodic) at their ends."""
    sig2 = _rows_signal('delay_rows', sig)
    return _spectral_rows_host(sig2, _delay_rows_terms(sig2.shape[0], delays), sample_rate)


def _shift_split(name, delays, dt):
    """delays (a list of numbers) -> (points, deltas) by the reference's own expressions (distortion.py:24-25):
    points = int(delay // dt), delta = delay / dt - points.  Python's floor division is not floor(delay / dt):
    1.0 // 0.1 is 9 and delta comes out as exactly 1.0, which the stage takes.  ValueError for a delay or dt that is
    not finite, dt = 0, or a split that leaves delta outside [0, 1]."""
    dt = float(dt)
    if not np.isfinite(dt) or dt == 0.0:
        raise ValueError(f'{name}: dt must be finite and not zero')
    points, deltas = [], []
    for r, d in enumerate(delays):
        d = float(d)
        if not np.isfinite(d):
            raise ValueError(f'{name}: row {r}: delay is not finite')
        p = int(d // dt)
        delta = d / dt - p
        if not 0.0 <= delta <= 1.0:
            raise ValueError(f'{name}: row {r}: delay / dt = {d / dt!r} does not split into whole samples and a fraction')
        points.append(p)
        deltas.append(delta)
    return points, deltas


class ShiftStage:
    """Device-resident per-row delay in time for `batch` rows of `n` samples (build once, apply many times): the
    reference's `shift(x[r], delays[r], dt)` (distortion.py:12-39) for every row, one skew per line.  With
    p = int(delay // dt) and d = delay / dt - p (the reference's expressions, evaluated here on the host):
        y[r, i] = (1 - d) x[r, i - p] + d x[r, i - p - 1]     samples outside [0, n) are zero, and so is y wherever
                                                              i - p is outside [0, n)
    and for d = 0 a plain zero-filled shift by p samples that moves values bit for bit (inf and NaN included).
    Linear interpolation, zero fill: not the circular band-limited `('delay', tau)` of `ReflectionStage`.
    Where the reference differs, on purpose: it returns 3 samples for n < 3 with a fractional delay (rows keep n
    here), and it multiplies x[i + 1] by a zero tap, so an inf there gives NaN at i (not here).
    `delays`: a scalar (every row; give `batch`) or one value per row.  float32 rows are computed in float64 and
    rounded once.  `.points` / `.deltas`: the split per row.

        st = ShiftStage(skews, n, 1 / 2e9)
        st.apply_torch(x, out=y)               # out of place, on torch's current stream
    """

    def __init__(self, delays, n: int, dt: float, dtype=np.float64, batch=None):
        scalar = np.ndim(delays) == 0
        if scalar and batch is None:
            raise ValueError('ShiftStage: a scalar delay needs batch=')
        rows = [delays] * int(batch) if scalar else list(np.asarray(delays).reshape(-1))
        if batch is not None and len(rows) != int(batch):
            raise ValueError(f'ShiftStage: {len(rows)} delays for {int(batch)} rows')
        if not rows:
            raise ValueError('ShiftStage: no rows')
        points, deltas = _shift_split('ShiftStage', rows, dt)
        self._set_plan(_engine.ShiftRowsPlan(points, deltas, n, dtype), float(dt))

    def _set_plan(self, plan, dt):
        self.plan, self.dt = plan, dt
        self.n, self.batch, self.dtype = plan.n, plan.batch, plan.dtype
        self.points, self.deltas = plan.points, plan.deltas

    @classmethod
    def from_split(cls, points, deltas, n: int, dtype=np.float64):
        """the stage of rows whose delays are already split: points[r] whole samples and deltas[r] in [0, 1] of one"""
        self = cls.__new__(cls)
        self._set_plan(_engine.ShiftRowsPlan(points, deltas, n, dtype), None)
        return self

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, stream=0):
        self.plan.apply(in_ptr, in_stride, out_ptr, out_stride, stream)

    def kernel_name(self) -> str:
        return self.plan.kernel_name()

    def apply_torch(self, x, out):
        """x, out: (batch, >= n) row-contiguous device tensors of the stage's dtype (rows may be windows of a wider
        tensor); out of place: the rows of `out` may share no memory with the rows of `x` (ValueError).
        Asynchronous on torch's current stream; one stage may serve several streams.  -> out"""
        import torch
        (x0, xs), (y0, ys) = (_rows.check_rows(
            t, self.batch, self.n, _rows.torch_dtype(self.dtype),
            'expected (batch, >=n) row-contiguous device tensors of the stage dtype') for t in (x, out))
        es = self.dtype.itemsize
        if not _rows.rows_disjoint((x0, xs, self.batch, self.n, es), (y0, ys, self.batch, self.n, es)):
            raise ValueError('shift is out of place: out overlaps x')
        self.apply(x0, xs, y0, ys, torch.cuda.current_stream(x.device).cuda_stream)
        return out

    def close(self):
        self.plan.close()


def shift_rows(sig, delays, dt):
    """`shift(sig[r], delays[r], dt)` for every row r of a 2-D `sig` (reference distortion.py:12-39 per row; `delays`
    a scalar: every row), all rows in one launch: see `ShiftStage` for the formula and the two places where rows of
    fewer than 3 samples or with inf in them differ from the reference.  float32 rows stay float32, anything else
    is computed as float64.  ValueError before any device work: sig not 2-D, a number of delays that does not match,
    a delay that is not finite.  NotImplementedError: complex rows."""
    sig2 = _rows_signal_f32('shift_rows', sig)
    batch, n = sig2.shape
    points, deltas = _shift_split('shift_rows', _per_row('shift_rows', 'delay', delays, batch), dt)
    if n == 0 or batch == 0:
        return sig2.copy()
    with _engine.ShiftRowsPlan(points, deltas, n, sig2.dtype) as plan, _engine.DeviceBuffer(sig2.nbytes) as x, \
            _engine.DeviceBuffer(sig2.nbytes) as y:
        x.upload(sig2)
        plan.apply(x.ptr, n, y.ptr, n)
        _engine.sync()
        return y.download(sig2.shape, sig2.dtype)


class MixStage:
    """Device-resident linear mixing ACROSS rows, per sample (build once, apply many times): `rows_in` rows of `n`
    samples become `rows_out` rows through a sparse `matrix` (rows_out, rows_in) and an `offset` per output row -- flux
    crosstalk compensation (the inverse of the measured crosstalk matrix, a band), IQ mixer correction (a 2 x 2 block per
    pair and a DC offset against carrier leakage).  A TERM of output row o is an entry M[o, c] != 0; in float64 (a
    float32 sample is widened first), product and sum each rounded (no fused multiply-add), terms in ascending c:
        acc = 0.0;   acc = acc + x[c, i] * M[o, c]  for every term;   y[o, i] = acc + offset[o]
    -- bit for bit what that NumPy loop gives; a float32 result is rounded once at the end.  A row of x on which o has
    no term is not read for o: its NaN and inf stay out of y[o] (a dense product would make them NaN).
    `matrix`: a 2-D array-like or a scipy.sparse matrix; `offset`: None (zeros) or one value per output row.
    `.rows_out`, `.rows_in`, `.nnz` (the terms); `.reads`: the input rows the kernel reads, every tile of
    `_engine.MIX_TILE_ROWS` consecutive output rows reading each row it has a term on once -- rows_in for blocks that
    divide the tile, about (T + 2 k) / T * rows_in for a band of half-width k, rows_in * tiles for a dense matrix:
    put coupled lines next to each other.

        st = MixStage(np.linalg.inv(crosstalk), n)              # or MixStage.from_blocks([[[a, b], [c, d]], ...], n)
        st.apply_torch(x, out=y)                                # out of place, on torch's current stream
    """

    def __init__(self, matrix, n: int, offset=None, dtype=np.float64):
        self.plan = _engine.MixRowsPlan(matrix, offset, n, dtype)
        p = self.plan
        self.n, self.dtype, self.offset = p.n, p.dtype, p.offset
        self.rows_out, self.rows_in, self.nnz, self.reads = p.rows_out, p.rows_in, p.nnz, p.reads

    @staticmethod
    def block_diagonal(blocks):
        """the dense matrix with the 2-D `blocks` down its diagonal (they need not be square)"""
        blocks = [np.asarray(b, dtype=np.float64) for b in blocks]
        if not blocks or any(b.ndim != 2 for b in blocks):
            raise ValueError('MixStage: blocks is a list of 2-D arrays, at least one')
        m = np.zeros((sum(b.shape[0] for b in blocks), sum(b.shape[1] for b in blocks)))
        r = c = 0
        for b in blocks:
            m[r:r + b.shape[0], c:c + b.shape[1]] = b
            r, c = r + b.shape[0], c + b.shape[1]
        return m

    @classmethod
    def from_blocks(cls, blocks, n: int, offset=None, dtype=np.float64):
        """the stage of the block-diagonal matrix of a list of small 2-D arrays: [[a, b], [c, d]] per IQ pair gives
        I' = a I + b Q, Q' = c I + d Q"""
        return cls(cls.block_diagonal(blocks), n, offset, dtype)

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, stream=0):
        self.plan.apply(in_ptr, in_stride, out_ptr, out_stride, stream)

    def kernel_name(self) -> str:
        return self.plan.kernel_name()

    def apply_torch(self, x, out=None):
        """x: (rows_in, >= n), out: (rows_out, >= n) row-contiguous device tensors of the stage's dtype (rows may be
        windows of a wider tensor; out None: allocated); out of place: the rows of `out` may share no memory with the
        rows of `x` (ValueError), and `x` is never written.  Asynchronous on torch's current stream.  -> out"""
        import torch
        tdt = _rows.torch_dtype(self.dtype)
        x0, xs = _rows.check_rows(x, self.rows_in, self.n, tdt,
                                  'expected x: (rows_in, >=n) row-contiguous device tensor of the stage dtype')
        if out is None:
            out = torch.empty((self.rows_out, self.n), dtype=tdt, device=x.device)
        y0, ys = _rows.check_rows(out, self.rows_out, self.n, tdt,
                                  'expected out: (rows_out, >=n) row-contiguous device tensor of the stage dtype')
        es = self.dtype.itemsize
        if not _rows.rows_disjoint((x0, xs, self.rows_in, self.n, es), (y0, ys, self.rows_out, self.n, es)):
            raise ValueError('mix stage is out of place: out overlaps x')
        self.apply(x0, xs, y0, ys, torch.cuda.current_stream(x.device).cuda_stream)
        return out

    def close(self):
        self.plan.close()


def mix_rows(sig, matrix, offset=None):
    """`matrix` applied across the rows of a 2-D real `sig`, per sample, plus `offset` per output row (see `MixStage`
    for the formula), in one launch: NumPy in, NumPy out, (rows of the matrix, samples).  float32 rows stay float32,
    anything else is computed as float64.  ValueError before any device work: sig not 2-D, a matrix whose columns are
    not the rows of sig, what `MixStage` refuses.  NotImplementedError: complex rows."""
    sig2 = _rows_signal_f32('mix_rows', sig)
    batch, n = sig2.shape
    rows_in, row_ptr, col, val, off, n, dtype = _engine._mix_rows_checked(matrix, offset, n, sig2.dtype)
    if rows_in != batch:
        raise ValueError(f'mix_rows: a matrix of {rows_in} columns for {batch} rows')
    rows_out = len(row_ptr) - 1
    if n == 0:
        return np.zeros((rows_out, 0), dtype=dtype)
    with _engine.MixRowsPlan(matrix, offset, n, dtype) as plan, _engine.DeviceBuffer(sig2.nbytes) as x, \
            _engine.DeviceBuffer(rows_out * n * dtype.itemsize) as y:
        x.upload(sig2)
        plan.apply(x.ptr, n, y.ptr, n)
        _engine.sync()
        return y.download((rows_out, n), dtype)


class DacStage:
    """Device-resident volts -> DAC codes for `batch` rows of `n` samples (build once, apply many times): the last
    step before an upload to an AWG.  Input row r has `gain[r]` (LSB per unit of the signal) and `offset[r]` (LSB);
    in float64 (a float32 sample is widened first), product and sum each rounded (no fused multiply-add):
        v = x[r, i] * gain[r] + offset[r];   q = rint(v), half to even;   lo = -2**(bits - 1), hi = 2**(bits - 1) - 1
        c = 0 where v is NaN, lo where q < lo, hi where q > hi, q otherwise;   code = c * 2**shift as int16
    (`shift` left-justifies a 12/14-bit converter in its 16-bit word).  `interleave=2` packs the rows [I, Q] of a pair
    into one output row I0 Q0 I1 Q1 ...: `.out_rows = batch // interleave` rows of `.out_n = interleave * n` codes.
    `gain` / `offset`: a scalar (every row; give `batch`) or one value per INPUT row.  An optional (batch, 3) int64
    counts tensor is OVERWRITTEN by every apply with [below, above, nan] per input row: how many samples clipped.

        st = DacStage.from_full_scale(1.0, n, batch=rows)       # +-1.0 -> +-32767
        codes = st.apply_torch(z, counts=clipped)               # out of place, on torch's current stream
    """

    def __init__(self, gain, n: int, offset=0.0, bits: int = 16, shift: int = 0, interleave: int = 1,
                 dtype=np.float64, batch=None):
        if np.ndim(gain) == 0 and np.ndim(offset) == 0 and batch is None:
            raise ValueError('DacStage: a scalar gain and offset need batch=')
        if batch is None:
            batch = np.size(gain) if np.ndim(gain) > 0 else np.size(offset)
        batch = int(batch)
        if batch < 1:
            raise ValueError('DacStage: no rows')
        gains, offsets = _gain_offset_rows('DacStage', gain, offset, batch)
        self.plan = _engine.DacRowsPlan(gains, offsets, n, bits, shift, interleave, dtype)
        p = self.plan
        self.n, self.batch, self.dtype, self.gain, self.offset = p.n, p.batch, p.dtype, p.gain, p.offset
        self.bits, self.shift, self.interleave = p.bits, p.shift, p.interleave
        self.lo, self.hi, self.out_rows, self.out_n = p.lo, p.hi, p.out_rows, p.out_n

    @classmethod
    def from_full_scale(cls, full_scale_rows, n: int, **kw):
        """the stage whose gain[r] = hi / full_scale_rows[r], so that +-full scale maps to +-hi (a scalar: every row;
        give `batch`).  ValueError: a full scale that is not finite or not positive."""
        return cls(_full_scale_gain('DacStage', full_scale_rows, kw), n, **kw)

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, stream=0):
        self.plan.apply(in_ptr, in_stride, out_ptr, out_stride, counts_ptr, stream)

    def kernel_name(self, counts: bool = False) -> str:
        return self.plan.kernel_name(counts)

    def apply_torch(self, x, out=None, counts=None):
        """x: (batch, >= n) row-contiguous device tensor of the stage's dtype; out: (out_rows, >= out_n) int16 (rows
        may be windows of a wider tensor; None: allocated); counts: None or a contiguous (batch, 3) int64 device
        tensor, overwritten.  Out of place: `out` may share no memory with `x`, `counts` with neither (ValueError);
        `x` is never written.  Asynchronous on torch's current stream.  -> out[:, :out_n]"""
        import torch
        x0, xs = _rows.check_rows(x, self.batch, self.n, _rows.torch_dtype(self.dtype),
                                  'expected x: (batch, >=n) row-contiguous device tensor of the stage dtype')
        if out is None:
            out = torch.empty((self.out_rows, self.out_n), dtype=torch.int16, device=x.device)
        y0, ys = _rows.check_rows(out, self.out_rows, self.out_n, torch.int16,
                                  'expected out: (out_rows, >=out_n) row-contiguous int16 device tensor')
        sides = (x0, xs, self.batch, self.n, self.dtype.itemsize), (y0, ys, self.out_rows, self.out_n, 2)
        c0 = _check_reports('dac stage', 'out', 'batch', self.batch, sides, counts)[0]
        self.apply(x0, xs, y0, ys, c0, torch.cuda.current_stream(x.device).cuda_stream)
        return out[:, :self.out_n]

    def close(self):
        self.plan.close()


def dac_codes_rows(sig, gain, offset=0.0, bits=16, shift=0, interleave=1, return_counts=False):
    """The int16 DAC codes of every row of a 2-D real `sig` (see `DacStage` for the formula), all rows in one launch:
    NumPy in, NumPy out, (rows // interleave, interleave * samples).  `gain` / `offset`: a scalar (every row) or one
    value per row.  float32 rows stay float32 on the way in, anything else is read as float64.  `return_counts`:
    -> (codes, counts), counts the (rows, 3) int64 [below, above, nan] per input row.  ValueError before any device
    work: sig not 2-D, a number of gains or offsets that does not match, what `DacStage` refuses.
    NotImplementedError: complex rows."""
    sig2 = _rows_signal_f32('dac_codes_rows', sig)
    batch, n = sig2.shape
    gains = _per_row('dac_codes_rows', 'gain', gain, batch)
    offsets = _per_row('dac_codes_rows', 'offset', offset, batch)
    g, o, n, bits, shift, k, dtype = _engine.dac_rows_arguments(gains, offsets, n, bits, shift, interleave, sig2.dtype)
    return _one_shot(sig2, lambda: _engine.DacRowsPlan(g, o, n, bits, shift, k, dtype),
                     lambda plan, x, y, reports, levels: plan.apply(x, n, y, k * n, reports[0]),
                     shape=(batch // k, k * n), dtype=np.int16, report_rows=batch, reports=1,
                     return_counts=return_counts)


class MixDacStage:
    """`MixStage(matrix, n, mix_offset, dtype).apply_torch(x)` followed by `DacStage(gain, n, dac_offset, bits, shift,
    interleave, dtype, batch=rows_out).apply_torch(., counts=)`, device-resident and bit for bit -- codes and counts --
    in ONE kernel ('mix_dac_rows<T,K,COUNT>') without the float rows between the two: the inverse crosstalk matrix of
    the flux lines, or the 2 x 2 mixer correction and DC offset of every IQ pair, ending in the int16 codes of the
    converter.  In float64, product and sum each rounded, terms in ascending column (see `MixStage`, `DacStage`):
        y = sum of x[c, i] * M[o, c] + mix_offset[o]       (a float32 plan rounds y to float32 once, as the two stages)
        code[o, i] = saturate(rint(y * gain[o] + dac_offset[o])) * 2**shift;   out[g, i * k + j] = code[g * k + j, i]
    `gain` / `dac_offset`: a scalar (every row) or one value per OUTPUT row of the matrix; `interleave=2` packs the mixed
    rows [I, Q] of a pair into one code row I0 Q0 I1 Q1 ...  An optional (rows_out, 3) int64 counts tensor is OVERWRITTEN
    by every apply with [below, above, nan] per mixed row.  `.rows_out`, `.rows_in`, `.nnz`; `.reads`: the input rows
    the kernel reads at its tile height `_engine.MIX_DAC_TILE_ROWS`; `.span`: the codes of one row a workgroup covers;
    `.out_rows`, `.out_n`, `.lo`, `.hi`, `.gain`, `.offset` (the DAC's; `.mix_offset`: the mix's).

        st = MixDacStage.from_blocks([[[a, b], [c, d]], ...], n, gain, mix_offset=leak, interleave=2)
        codes = st.apply_torch(x, counts=clipped)               # out of place, on torch's current stream
    """

    def __init__(self, matrix, n: int, gain, mix_offset=None, dac_offset=0.0, bits: int = 16, shift: int = 0,
                 interleave: int = 1, dtype=np.float64):
        rows_out = _engine._mix_rows_csr(matrix)[0]
        gains, offsets = (_gain_offset_rows('MixDacStage', gain, dac_offset, rows_out) if rows_out >= 1
                          else ([0.0], [0.0]))
        self.plan = _engine.MixDacPlan(matrix, mix_offset, gains, offsets, n, bits, shift, interleave, dtype)
        p = self.plan
        self.n, self.dtype, self.mix_offset, self.gain, self.offset = p.n, p.dtype, p.mix_offset, p.gain, p.dac_offset
        self.rows_out, self.rows_in, self.nnz, self.reads = p.rows_out, p.rows_in, p.nnz, p.reads
        self.bits, self.shift, self.interleave = p.bits, p.shift, p.interleave
        self.lo, self.hi, self.out_rows, self.out_n = p.lo, p.hi, p.out_rows, p.out_n
        self.span = p.span()

    @classmethod
    def from_blocks(cls, blocks, n: int, gain, **kw):
        """the stage of the block-diagonal matrix of a list of small 2-D arrays (`MixStage.from_blocks`)"""
        return cls(MixStage.block_diagonal(blocks), n, gain, **kw)

    @classmethod
    def from_full_scale(cls, matrix, n: int, full_scale, **kw):
        """the stage whose gain[o] = hi / full_scale[o], so that a mixed +-full scale maps to +-hi (a scalar: every
        row).  ValueError: a full scale that is not finite or not positive."""
        return cls(matrix, n, _full_scale_gain('MixDacStage', full_scale, kw), **kw)

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, stream=0):
        self.plan.apply(in_ptr, in_stride, out_ptr, out_stride, counts_ptr, stream)

    def kernel_name(self, counts: bool = False) -> str:
        return self.plan.kernel_name(counts)

    def apply_torch(self, x, out=None, counts=None):
        """x: (rows_in, >= n) row-contiguous device tensor of the stage's dtype; out: (out_rows, >= out_n) int16 (rows
        may be windows of a wider tensor; None: allocated); counts: None or a contiguous (rows_out, 3) int64 device
        tensor, overwritten.  Out of place: `out` may share no memory with `x`, `counts` with neither (ValueError);
        `x` is never written.  Asynchronous on torch's current stream.  -> out[:, :out_n]"""
        import torch
        x0, xs = _rows.check_rows(x, self.rows_in, self.n, _rows.torch_dtype(self.dtype),
                                  'expected x: (rows_in, >=n) row-contiguous device tensor of the stage dtype')
        if out is None:
            out = torch.empty((self.out_rows, self.out_n), dtype=torch.int16, device=x.device)
        y0, ys = _rows.check_rows(out, self.out_rows, self.out_n, torch.int16,
                                  'expected out: (out_rows, >=out_n) row-contiguous int16 device tensor')
        sides = (x0, xs, self.rows_in, self.n, self.dtype.itemsize), (y0, ys, self.out_rows, self.out_n, 2)
        c0 = _check_reports('mix dac stage', 'out', 'rows_out', self.rows_out, sides, counts)[0]
        self.apply(x0, xs, y0, ys, c0, torch.cuda.current_stream(x.device).cuda_stream)
        return out[:, :self.out_n]

    def close(self):
        self.plan.close()


def mix_dac_rows(sig, matrix, gain, mix_offset=None, dac_offset=0.0, bits=16, shift=0, interleave=1,
                 return_counts=False):
    """`dac_codes_rows(mix_rows(sig, matrix, mix_offset), gain, dac_offset, bits, shift, interleave)` in one launch
    (see `MixDacStage`): NumPy in, NumPy out, (rows of the matrix // interleave, interleave * samples) int16.  float32
    rows stay float32 on the way in, anything else is read as float64.  `return_counts`: -> (codes, counts), counts the
    (rows of the matrix, 3) int64 [below, above, nan].  ValueError before any device work: sig not 2-D, a matrix whose
    columns are not the rows of sig, what `MixDacStage` refuses.  NotImplementedError: complex rows."""
    sig2 = _rows_signal_f32('mix_dac_rows', sig)
    batch, n = sig2.shape
    rows_out = _engine._mix_rows_csr(matrix)[0]
    gains = _per_row('mix_dac_rows', 'gain', gain, max(rows_out, 1))
    offsets = _per_row('mix_dac_rows', 'offset', dac_offset, max(rows_out, 1))
    rows_in = _engine.mix_dac_arguments(matrix, mix_offset, gains, offsets, n, bits, shift, interleave, sig2.dtype)[0]
    if rows_in != batch:
        raise ValueError(f'mix_dac_rows: a matrix of {rows_in} columns for {batch} rows')
    k = int(interleave)
    return _one_shot(sig2, lambda: _engine.MixDacPlan(matrix, mix_offset, gains, offsets, n, bits, shift, k, sig2.dtype),
                     lambda plan, x, y, reports, levels: plan.apply(x, n, y, k * n, reports[0]),
                     shape=(rows_out // k, k * n), dtype=np.int16, report_rows=rows_out, reports=1,
                     return_counts=return_counts)


class IirDacStage:
    """`IirStage(sections_rows, n, batch, dtype).apply_torch(x, out=z, initial=, zi=, zf=)` followed by `DacStage(gain, n,
    offset, bits, shift, dtype=dtype).apply_torch(z, counts=)`, device-resident and bit for bit -- codes, counts and
    zf -- in ONE kernel ('iir_rows_dac<T,NSEC,ORD>') without the float rows between the two: a flux line without a
    crosstalk matrix, whose last float stage is its own exp-decay correction, ending in the int16 codes of the
    converter.  Row r, with `IirStage`'s per-row rules (cascades padded to a common shape: sections of equal order,
    total state dimension <= 4) and `DacStage`'s formula:
        y = F_r(x[r] - initial[r]) + initial[r]            (a float32 plan rounds y to float32 once, as the two stages)
        code[r, i] = saturate(rint(y[i] * gain[r] + offset[r])) * 2**shift
    `sections_rows`: one cascade [(b, a), ...] per row; ONE cascade -- [(b, a), ...] or an SOS matrix -- is given to
    every row (`batch=`, or the number of gains).  `gain` / `offset`: a scalar (every row) or one value per row.  An
    optional (batch, 3) int64 counts tensor is OVERWRITTEN by every apply with [below, above, nan] per row.
    `interleave` is not part of this stage (NotImplementedError: a pair is `IirStage` + `DacStage(interleave=2)`).

        st = IirDacStage.from_full_scale([[exp_decay_filter(A, tau, 2e9)] for A, tau in lines], n, 1.0)
        codes = st.apply_torch(x, counts=clipped, initial=levels, zf=zf)     # out of place, torch's current stream
    """

    def __init__(self, sections_rows, n: int, gain, offset=0.0, bits: int = 16, shift: int = 0, dtype=np.float64,
                 interleave: int = 1, batch=None):
        if interleave != 1:
            raise NotImplementedError('IirDacStage has no interleave: a workgroup owns one row; run IirStage and then '
                                      'DacStage(interleave=2) for a pair')
        sections_rows, _ = _cascade_rows(
            'IirDacStage', sections_rows, batch, 'one [(b, a), ...] per row, one [(b, a), ...], or an SOS matrix',
            one_for=_given_rows(gain, offset))
        gains, offsets = _gain_offset_rows('IirDacStage', gain, offset, len(sections_rows))
        self.plan = _engine.IirRowsDacPlan(sections_rows, gains, offsets, n, bits, shift, dtype)
        p = self.plan
        self.n, self.batch, self.dtype, self.gain, self.offset = p.n, p.batch, p.dtype, p.gain, p.offset
        self.bits, self.shift, self.lo, self.hi = p.bits, p.shift, p.lo, p.hi
        self.state_dim, self.own_orders, self.section_order = p.state_dim, p.own_orders, int(p.orders[0])
        self._initial_cache = None

    @classmethod
    def from_full_scale(cls, sections_rows, n: int, full_scale, **kw):
        """the stage whose gain[r] = hi / full_scale[r], so that a filtered +-full scale maps to +-hi (a scalar: every
        row).  ValueError: a full scale that is not finite or not positive."""
        return cls(sections_rows, n, _full_scale_gain('IirDacStage', full_scale, kw), **kw)

    def kernel_name(self) -> str:
        """'iir_rows_dac<T,NSEC,ORD>'"""
        return self.plan.kernel_name()

    def row_state(self, z, r: int):
        """row r's own state (scipy layout, its sections back to back) out of a (batch, state_dim) host array"""
        return _row_state(z, r, self.own_orders, self.section_order)

    def apply_torch(self, x, codes=None, counts=None, initial=0.0, zi=None, zf=None):
        """x: (batch, >= n) row-contiguous device tensor of the stage's dtype -- or ONE row, (1, >= n) or 1-D, that
        every row reads (the shared-input form); codes: (batch, >= n) int16 (rows may be windows of a wider tensor;
        None: allocated); counts: None or a contiguous (batch, 3) int64 device tensor, overwritten; `initial`: a
        scalar, one value per row, or a (batch,) float64 device tensor; zi / zf: optional (batch, state_dim) float64
        device tensors.  Out of place: `codes` may share no memory with `x`, `counts` with neither (ValueError); `x`
        is never written.  Asynchronous on torch's current stream.  -> codes[:, :n]"""
        import torch
        if x.dim() == 1:
            x = x.unsqueeze(0)
        shared = self.batch > 1 and x.shape[0] == 1
        in_rows = 1 if shared else self.batch
        x0, xs = _rows.check_rows(x, in_rows, self.n, _rows.torch_dtype(self.dtype),
                                  'expected x: (batch, >=n) row-contiguous device tensor of the stage dtype, or one row')
        if codes is None:
            codes = torch.empty((self.batch, self.n), dtype=torch.int16, device=x.device)
        y0, ys = _rows.check_rows(codes, self.batch, self.n, torch.int16,
                                  'expected codes: (batch, >=n) row-contiguous int16 device tensor')
        sides = (x0, xs, in_rows, self.n, self.dtype.itemsize), (y0, ys, self.batch, self.n, 2)
        c0, _, zip_, zfp = _check_reports('iir dac stage', 'codes', 'batch', self.batch, sides, counts,
                                          zi=zi, zf=zf, state_dim=self.state_dim)
        ini = _initial_rows(self, self.batch, initial, x.device)
        inip = None if ini is None else ini.data_ptr()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if shared:
            self.plan.apply_shared_in(x0, y0, ys, c0, zip_, zfp, inip, stream)
        else:
            self.plan.apply(x0, xs, y0, ys, c0, zip_, zfp, inip, stream)
        return codes[:, :self.n]

    def close(self):
        self.plan.close()


def iir_dac_rows(sig, filters_rows, gain, offset=0.0, bits=16, shift=0, initial=0.0, return_counts=False):
    """`dac_codes_rows(<IirStage of one cascade per row>(sig, initial=initial), gain, offset, bits, shift)` in one
    launch (see `IirDacStage`): NumPy in, NumPy out, (rows, samples) int16.  `filters_rows`: one list of (b, a)
    sections per row (run as a cascade, in `IirStage`'s per-row shapes); `initial`: a scalar or one level per row.
    float32 rows stay float32 on the way in, anything else is read as float64.  `return_counts`: -> (codes, counts),
    counts the (rows, 3) int64 [below, above, nan].  ValueError before any device work: sig not 2-D, a number of
    cascades, gains, offsets or levels that does not match, what `IirDacStage` refuses.  NotImplementedError: complex
    rows or coefficients."""
    sig2 = _rows_signal_f32('iir_dac_rows', sig)
    batch, n = sig2.shape
    filters_rows = [list(f) for f in filters_rows]
    if len(filters_rows) != batch:
        raise ValueError(f'iir_dac_rows: {len(filters_rows)} filter lists for {batch} rows')
    gains = _per_row('iir_dac_rows', 'gain', gain, batch)
    offsets = _per_row('iir_dac_rows', 'offset', offset, batch)
    g, o, n, bits, shift, _, dtype = _engine.dac_rows_arguments(gains, offsets, n, bits, shift, 1, sig2.dtype)
    packed = _engine.pack_sections_rows(filters_rows)
    ini = _initial_host(initial, batch, 'iir_dac_rows: initial is a scalar or one value per row')
    return _one_shot(sig2, lambda: _engine.IirRowsDacPlan(filters_rows, g, o, n, bits, shift, dtype, packed=packed),
                     lambda plan, x, y, reports, levels: plan.apply(x, n, y, n, reports[0], None, None, levels),
                     shape=(batch, n), dtype=np.int16, report_rows=batch, reports=1, return_counts=return_counts,
                     initial=ini)


class SampledDac(_LentScratch):
    """`BatchSampler(channels, grid).launch_torch(z)` (float64) followed by `DacStage(gain, n, offset, ...)
    .apply_torch(z)`, device-resident and bit for bit -- codes and counts -- with the float64 rows left out: a
    microwave drive line has no predistortion between its waveform and its converter, so at AWG sample rates the
    sampler's own kernel scales, rounds, saturates and stores the int16 codes (`fused`; `kernel_name()` is
    'wfk_sample_short_dac<16,FAM,COUNT>'): 2 B per sample of HBM traffic instead of 8 written, 8 read and 2 written.
    Plans the fused kernel does not take (`why_not`: long pieces, mixed plans, `interleave=2`, WFK_CHAIN_UNFUSED=1)
    run the two launches through a float64 scratch taken once, here.  `gain` / `offset`: a scalar or one value per
    channel; `bits`, `shift`, `interleave` and the optional (n_channels, 3) int64 counts as `DacStage` has them.
    Build once, launch many times.

        sd = SampledDac.from_full_scale(channels, wl.awg_grid(n, 2e9), 1.0)      # +-1.0 -> +-32767
        sd.launch_torch(codes, counts=clipped)       # (n_channels, >= n) int16 device tensor, torch's current stream
    """

    def __init__(self, channels, grid, gain, offset=0.0, bits: int = 16, shift: int = 0, interleave: int = 1,
                 function_lib=None, tile=1):
        """`tile` > 1 repeats the channel list that many times (synthetic batches, as BatchSampler's)"""
        from . import _flatten
        channels = list(channels)
        rows = len(channels) * max(int(tile), 1)
        if rows < 1:
            raise ValueError('SampledDac: no rows')
        gains, offsets = _gain_offset_rows('SampledDac', gain, offset, rows)
        if not isinstance(grid, _flatten.wfk_grid):
            grid = _flatten.grid_from_desc(grid)
        # argument errors before any device work
        _engine.dac_rows_arguments(gains, offsets, int(grid.n), bits, shift, interleave)
        self.prog = _flatten.tile_program(_flatten.flatten(channels, grid, function_lib), tile)
        if self.prog.n_channels != rows:
            raise ValueError(f'SampledDac: {rows} gains for {self.prog.n_channels} rows')
        if self.prog.complex_amp or self.prog.host_complex:
            raise NotImplementedError('complex rows')
        self.plan = _engine.ChainDacPlan(self.prog, grid, gains, offsets, bits, shift, interleave)
        p = self.plan
        self.n, self.n_channels, self.gain, self.offset = p.n, p.n_channels, p.gain, p.offset
        self.bits, self.shift, self.interleave = p.bits, p.shift, p.interleave
        self.lo, self.hi, self.out_rows, self.out_n = p.lo, p.hi, p.out_rows, p.out_n
        self.fused, self.why_not = p.fused, p.why_not
        self._take_scratch()                                       # the unfused path's float64 rows: taken once, here

    @classmethod
    def from_full_scale(cls, channels, grid, full_scale, **kw):
        """the plan whose gain[r] = hi / full_scale[r], so that +-full scale maps to +-hi (a scalar: every row).
        ValueError: a full scale that is not finite or not positive."""
        return cls(channels, grid, _full_scale_gain('SampledDac', full_scale, kw), **kw)

    def kernel_name(self, counts: bool = False) -> str:
        """'wfk_sample_short_dac<16,FAM,COUNT>' | '<sampler kernels> + dac_rows<double>' (dac_rows_count with counts)"""
        return self.plan.kernel_name(counts)

    def launch(self, out_ptr, out_stride=None, counts_ptr=None, stream=0):
        """raw pointers; out_stride in codes (None: out_n)"""
        s = self._scratch
        self.plan.launch(out_ptr, self.out_n if out_stride is None else out_stride, counts_ptr,
                         None if s is None else s.ptr, self.n, stream)

    def launch_torch(self, codes, counts=None):
        """codes: (n_channels // interleave, >= interleave * n) row-contiguous int16 device tensor (rows may be a window
        of a wider tensor); counts: None or a contiguous (n_channels, 3) int64 device tensor, overwritten with [below,
        above, nan] per channel; it may share no memory with `codes` (ValueError).  Asynchronous on torch's current
        stream.  -> codes[:, :out_n]"""
        import torch
        y0, ys = _rows.check_rows(codes, self.out_rows, self.out_n, torch.int16,
                                  'expected codes: (out_rows, >=out_n) row-contiguous int16 device tensor')
        c0 = _check_reports('sampled dac', 'codes', 'n_channels', self.n_channels,
                            ((y0, ys, self.out_rows, self.out_n, 2), ), counts)[0]
        self.launch(y0, ys, c0, torch.cuda.current_stream(codes.device).cuda_stream)
        return codes[:, :self.out_n]

    def to_host(self, return_counts=False):
        """NumPy codes (out_rows, out_n) [, counts (n_channels, 3)]"""
        return _host_trip(lambda y, reports, dzi, dzf, levels: self.launch(y, None, reports[0]),
                          shape=(self.out_rows, self.out_n), dtype=np.int16, rows=self.n_channels,
                          reports=(return_counts, ))


class SampledIirDac(_LentScratch):
    """`SampledIirRows(channels, grid, filters_rows).launch_torch(z, initial=, zi=, zf=)` (float64) followed by
    `DacStage(gain, n, offset, bits, shift).apply_torch(z, counts=)`, device-resident and bit for bit -- codes, counts
    and zf -- with the float64 rows left out: a whole flux line, waveform, exp-decay correction and converter, in ONE
    kernel with 2 B per sample of HBM traffic.  Where `SampledIirRows` fuses (`fused`), the same fill runs in front of
    the codes store: `kernel_name()` is 'iir_rows_sampled_dac<f64,NSEC,ORD>' on fine grids,
    'iir_rows_short_dac<f64,NSEC,ORD>' at AWG sample rates.  Plans it does not take (`why_not`: clip on a fine grid,
    generic terms, WFK_CHAIN_UNFUSED=1) run the sampler into a float64 scratch taken once, here, and then
    'iir_rows_dac<f64,NSEC,ORD>': two launches instead of three.  `filters_rows`: one cascade [(b, a), ...] per row with
    `IirStage`'s per-row rules; `gain` / `offset`: a scalar or one value per channel; `bits`, `shift` and the optional
    (n_channels, 3) int64 counts as `DacStage` has them.  Build once, launch many times.

        sd = SampledIirDac.from_full_scale(channels, wl.awg_grid(n, 2e9), filters_rows, 1.0)     # +-1.0 -> +-32767
        sd.launch_torch(codes, counts=clipped, initial=levels, zf=zf)    # (n_channels, >= n) int16, the current stream
    """

    def __init__(self, channels, grid, filters_rows, gain, offset=0.0, bits: int = 16, shift: int = 0,
                 function_lib=None, tile=1):
        """`tile` > 1 repeats the channel list that many times (synthetic batches, as BatchSampler's)"""
        from . import _flatten
        channels, filters_rows = list(channels), list(filters_rows)
        rows = len(channels) * max(int(tile), 1)
        if rows < 1:
            raise ValueError('SampledIirDac: no rows')
        if len(filters_rows) != rows:
            raise ValueError(f'SampledIirDac: {len(filters_rows)} cascades for {rows} rows')
        gains, offsets = _gain_offset_rows('SampledIirDac', gain, offset, rows)
        if not isinstance(grid, _flatten.wfk_grid):
            grid = _flatten.grid_from_desc(grid)
        # argument errors before any device work
        _engine.dac_rows_arguments(gains, offsets, int(grid.n), bits, shift, 1)
        packed = _engine.pack_sections_rows(filters_rows)
        self.prog = _flatten.tile_program(_flatten.flatten(channels, grid, function_lib), tile)
        if self.prog.n_channels != rows:
            raise ValueError(f'SampledIirDac: {rows} cascades for {self.prog.n_channels} rows')
        if self.prog.complex_amp or self.prog.host_complex:
            raise NotImplementedError('complex rows')
        self.plan = _engine.ChainIirRowsDacPlan(self.prog, grid, filters_rows, gains, offsets, bits, shift, packed=packed)
        p = self.plan
        self.n, self.n_channels, self.gain, self.offset = p.n, p.n_channels, p.gain, p.offset
        self.bits, self.shift, self.lo, self.hi = p.bits, p.shift, p.lo, p.hi
        self.state_dim, self.own_orders, self.section_order = p.state_dim, packed[3], int(packed[0][0])
        self.fused, self.why_not = p.fused, p.why_not
        self._initial_cache = None
        self._take_scratch()                                       # the unfused path's float64 rows: taken once, here

    @classmethod
    def from_full_scale(cls, channels, grid, filters_rows, full_scale, **kw):
        """the plan whose gain[r] = hi / full_scale[r], so that a filtered +-full scale maps to +-hi (a scalar: every
        row).  ValueError: a full scale that is not finite or not positive."""
        return cls(channels, grid, filters_rows, _full_scale_gain('SampledIirDac', full_scale, kw), **kw)

    def row_state(self, z, r: int):
        """row r's own state (scipy layout, its sections back to back) out of a (n_channels, state_dim) host array"""
        return _row_state(z, r, self.own_orders, self.section_order)

    def kernel_name(self) -> str:
        """'iir_rows_sampled_dac<f64,NSEC,ORD>' | 'iir_rows_short_dac<f64,NSEC,ORD>' | '<sampler kernels> +
        iir_rows_dac<f64,NSEC,ORD>'"""
        return self.plan.kernel_name()

    def launch(self, out_ptr, out_stride=None, counts_ptr=None, zi_ptr=None, zf_ptr=None, initial_ptr=None, stream=0):
        """raw pointers; out_stride in codes (None: n); initial_ptr: device array of n_channels doubles or None"""
        s = self._scratch
        self.plan.launch(out_ptr, self.n if out_stride is None else out_stride, counts_ptr,
                         None if s is None else s.ptr, self.n, zi_ptr, zf_ptr, initial_ptr, stream)

    def launch_torch(self, codes, counts=None, initial=0.0, zi=None, zf=None):
        """codes: (n_channels, >= n) row-contiguous int16 device tensor (rows may be a window of a wider tensor);
        counts: None or a contiguous (n_channels, 3) int64 device tensor, overwritten with [below, above, nan] per
        channel; it may share no memory with `codes` (ValueError); `initial`: a scalar, one value per row, or a
        (n_channels,) float64 device tensor; zi / zf: optional (n_channels, state_dim) float64 device tensors.
        Asynchronous on torch's current stream.  -> codes[:, :n]"""
        import torch
        y0, ys = _rows.check_rows(codes, self.n_channels, self.n, torch.int16,
                                  'expected codes: (n_channels, >=n) row-contiguous int16 device tensor')
        c0, _, zip_, zfp = _check_reports('sampled iir dac', 'codes', 'n_channels', self.n_channels,
                                          ((y0, ys, self.n_channels, self.n, 2), ), counts,
                                          zi=zi, zf=zf, state_dim=self.state_dim)
        ini = _initial_rows(self, self.n_channels, initial, codes.device)
        self.launch(y0, ys, c0, zip_, zfp, None if ini is None else ini.data_ptr(),
                    torch.cuda.current_stream(codes.device).cuda_stream)
        return codes[:, :self.n]

    def to_host(self, initial=0.0, zi=None, return_counts=False, return_zf=False):
        """NumPy codes (n_channels, n) [, counts (n_channels, 3)] [, zf (n_channels, state_dim)]; initial: a scalar or
        one value per row; zi: (n_channels, state_dim)"""
        return _host_trip(lambda y, reports, dzi, dzf, levels: self.launch(y, None, reports[0], dzi, dzf, levels),
                          shape=(self.n_channels, self.n), dtype=np.int16, rows=self.n_channels,
                          reports=(return_counts, ), state_dim=self.state_dim, zi=zi, return_zf=return_zf,
                          initial=initial)


class CurveStage:
    """Device-resident calibration curve over sample VALUES for `batch` rows of `n` samples (build once, apply many
    times): a flux pulse programmed in its physical unit (detuning, flux) to volts through the line's measured
    monotone curve, an amplifier's compression table, a DAC's INL table.  Row r has knots `xp_rows[r]` (finite,
    strictly increasing, 2 .. `_engine.CURVE_MAX_KNOTS` of them; rows may differ in number) and values `fp_rows[r]`
    (finite); a sample below the first / above the last knot becomes `left[r]` / `right[r]` (any float, NaN too;
    default: the row's first / last value), a NaN sample stays that NaN.  In float64 (a float32 sample is widened
    first, the result rounded once), difference, product and sum each rounded (no fused multiply-add):
        y[r, i] = np.interp(x[r, i], xp_rows[r], fp_rows[r], left[r], right[r])           -- bit for bit.
    `xp_rows` / `fp_rows`: a list of 1-D arrays, a 2-D array, or one 1-D pair shared by `batch` rows; `left` /
    `right`: None, a scalar (every row) or one value per row.  `.batch`, `.n`, `.knots` (the knots per row).  An
    optional (batch, 3) int64 counts tensor is OVERWRITTEN by every apply with [below, above, nan] per row: how many
    samples left the measured range.

        st = CurveStage.inverse(volts, detuning, n)             # measured f(V), wanted V(f): one curve per line
        st.apply_torch(x, out=x)                                # in place (or out of place), on torch's current stream
    """

    def __init__(self, xp_rows, fp_rows, n: int, batch=None, left=None, right=None, dtype=np.float64):
        self.plan = _engine.CurveRowsPlan(xp_rows, fp_rows, n, batch, left, right, dtype)
        p = self.plan
        self.n, self.batch, self.dtype, self.knots = p.n, p.batch, p.dtype, p.knots
        self.left, self.right = p.left, p.right

    @staticmethod
    def inverse_rows(xp_rows, fp_rows):
        """the curves with the roles swapped -- knots `fp`, values `xp` -- rows whose `fp` descends reversed, so that
        the new knots ascend; ValueError names a row whose `fp` is not strictly monotone.  -> (xp_rows, fp_rows), lists"""
        xs, fs = _engine._curve_rows_list('xp', xp_rows), _engine._curve_rows_list('fp', fp_rows)
        if len(xs) != len(fs):
            raise ValueError(f'{len(xs)} rows of xp and {len(fs)} rows of fp')
        new_x, new_f = [], []
        for r, (x, f) in enumerate(zip(xs, fs)):
            if len(x) != len(f):
                raise ValueError(f'row {r}: {len(x)} knots and {len(f)} values')
            up, down = np.all(f[1:] > f[:-1]), np.all(f[1:] < f[:-1])
            if len(f) < 2 or not (up or down):
                raise ValueError(f'row {r}: values are not strictly monotone')
            new_x.append(f.copy() if up else f[::-1].copy())
            new_f.append(x.copy() if up else x[::-1].copy())
        return new_x, new_f

    @classmethod
    def inverse(cls, xp_rows, fp_rows, n: int, **kw):
        """the stage of the INVERSE curves: f(V) was measured at the points `xp_rows` with the results `fp_rows`, and
        V(f) is what the line needs.  Rows whose `fp_rows` descend are reversed; a row that is not strictly monotone is
        refused (ValueError, the row named).  Host work only, then the constructor's."""
        new_x, new_f = cls.inverse_rows(xp_rows, fp_rows)
        return cls(new_x, new_f, n, **kw)

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, stream=0):
        self.plan.apply(in_ptr, in_stride, out_ptr, out_stride, counts_ptr, stream)

    def kernel_name(self, counts: bool = False) -> str:
        return self.plan.kernel_name(counts)

    def apply_torch(self, x, out=None, counts=None):
        """x, out: (batch, >= n) row-contiguous device tensors of the stage's dtype (rows may be windows of a wider
        tensor; out None: allocated; `out is x`, or the same rows: in place); counts: None or a contiguous (batch, 3)
        int64 device tensor, overwritten.  Out of place the rows of `out` may share no memory with the rows of `x`,
        `counts` with neither (ValueError).  Asynchronous on torch's current stream.  -> out[:, :n]"""
        import torch
        tdt = _rows.torch_dtype(self.dtype)
        x0, xs = _rows.check_rows(x, self.batch, self.n, tdt,
                                  'expected x: (batch, >=n) row-contiguous device tensor of the stage dtype')
        if out is None:
            out = torch.empty((self.batch, self.n), dtype=tdt, device=x.device)
        y0, ys = _rows.check_rows(out, self.batch, self.n, tdt,
                                  'expected out: (batch, >=n) row-contiguous device tensor of the stage dtype')
        c0 = _rows.check_state(counts, (self.batch, 3), 'expected counts: contiguous (batch, 3) int64 device tensor',
                               dtype=np.int64)
        es = self.dtype.itemsize
        xr, yr = (x0, xs, self.batch, self.n, es), (y0, ys, self.batch, self.n, es)
        if not (x0 == y0 and xs == ys) and not _rows.rows_disjoint(xr, yr):
            raise ValueError('curve stage: out overlaps x without being x')
        if not _rows.report_disjoint(c0, self.batch, 3, xr, yr):
            raise ValueError('curve stage: counts overlaps x / out')
        self.apply(x0, xs, y0, ys, c0, torch.cuda.current_stream(x.device).cuda_stream)
        return out[:, :self.n]

    def close(self):
        self.plan.close()


def interp_rows(sig, xp_rows, fp_rows, left=None, right=None, return_counts=False):
    """np.interp(sig[r], xp_rows[r], fp_rows[r], left[r], right[r]) for every row of a 2-D real `sig`, all rows in one
    launch (see `CurveStage`): NumPy in, NumPy out.  float32 rows stay float32, anything else (integers too) is read as
    float64.  `xp_rows` / `fp_rows`: one curve per row, or one 1-D pair for every row.  `return_counts`: -> (y, counts),
    counts the (rows, 3) int64 [below, above, nan] per row.  ValueError before any device work: sig not 2-D, what
    `CurveStage` refuses.  NotImplementedError: complex rows.  A `sig` without samples is answered without a device."""
    sig2 = _rows_signal_f32('interp_rows', sig)
    batch, n = sig2.shape
    _engine.curve_rows_arguments(xp_rows, fp_rows, left, right, batch, n, sig2.dtype)   # every refusal comes first
    return _one_shot(sig2, lambda: _engine.CurveRowsPlan(xp_rows, fp_rows, n, batch, left, right, sig2.dtype),
                     lambda plan, x, y, reports, levels: plan.apply(x, n, y, n, reports[0]),
                     shape=None, dtype=None, report_rows=batch, reports=1, return_counts=return_counts)   # in place


class CurveIirDacStage:
    """`CurveStage(xp_rows, fp_rows, n, batch, left, right, dtype).apply_torch(x, out=v, counts=beyond)` followed by
    `IirDacStage(sections_rows, n, gain, offset, bits, shift, dtype).apply_torch(v, codes, counts, initial, zi, zf)`,
    device-resident and bit for bit -- codes, both reports and zf -- in ONE kernel ('iir_rows_curve_dac<T,NSEC,ORD>')
    without the float rows between them: a flux line programmed in its physical unit (detuning, flux), through the
    line's measured monotone curve to volts, its own exp-decay correction, and the converter.  Row r:
        v = np.interp(x[r], xp_rows[r], fp_rows[r], left[r], right[r])     (a float32 plan rounds v to float32 once)
        y = F_r(v - initial[r]) + initial[r]                               (`initial`: levels of v, in volts)
        code[r, i] = saturate(rint(y[i] * gain[r] + offset[r])) * 2**shift
    The curves follow `CurveStage`'s rules (2 .. 1024 finite, strictly increasing knots per row, finite values; rows may
    differ in number), the cascades `IirStage`'s per-row rules, gain / offset / bits / shift `DacStage`'s; a refusal
    names the curve first, then the converter, then the cascade.  Whoever measured f(V) and needs V(f) passes the
    output of `CurveStage.inverse_rows(volts, detuning)` as `xp_rows, fp_rows`.  The number of curves decides the rows
    (one 1-D pair: `batch=`, or the number of gains); ONE cascade is given to every row.  Two optional (batch, 3) int64
    reports are OVERWRITTEN by every apply: `beyond`, the curve's [below, above, nan] per row (samples outside the
    measured range), and `counts`, the converter's (codes that met a rail).  `interleave` is not part of this stage.
    What the stage saves is the float rows between the two (memory of the size of the batch) and a launch, not time: as
    measured the two stages are faster.

        xs, fs = CurveStage.inverse_rows(volts, detuning)
        st = CurveIirDacStage.from_full_scale(xs, fs, [[exp_decay_filter(A, tau, 2e9)] for A, tau in lines], n, 1.0)
        codes = st.apply_torch(x, counts=clipped, beyond=outside, initial=levels, zf=zf)
    """

    def __init__(self, xp_rows, fp_rows, sections_rows, n: int, gain, offset=0.0, bits: int = 16, shift: int = 0,
                 left=None, right=None, dtype=np.float64, batch=None, interleave: int = 1):
        if interleave != 1:
            raise NotImplementedError('CurveIirDacStage has no interleave: a workgroup owns one row; run CurveStage, '
                                      'IirStage and then DacStage(interleave=2) for a pair')
        xs = _engine._curve_rows_list('xp', xp_rows)
        if batch is None:
            batch = max(len(xs), _given_rows(gain, offset))
        curve = _engine.curve_rows_arguments(xp_rows, fp_rows, left, right, batch, n, dtype)   # the curve's rules first
        rows = len(curve[0]) - 1
        gains, offsets = _gain_offset_rows('CurveIirDacStage', gain, offset, rows)
        _engine.dac_rows_arguments(gains, offsets, n, bits, shift, 1, dtype)                    # then the converter's
        sections_rows, _ = _cascade_rows('CurveIirDacStage', sections_rows, rows,
                                         'one [(b, a), ...] per row, one [(b, a), ...], or an SOS matrix')
        self.plan = _engine.CurveIirDacPlan(xp_rows, fp_rows, sections_rows, gains, offsets, n, bits, shift, left, right,
                                            rows, dtype)
        p = self.plan
        self.n, self.batch, self.dtype, self.gain, self.offset = p.n, p.batch, p.dtype, p.gain, p.offset
        self.knots, self.left, self.right = p.knots, p.left, p.right
        self.bits, self.shift, self.lo, self.hi = p.bits, p.shift, p.lo, p.hi
        self.state_dim, self.own_orders, self.section_order = p.state_dim, p.own_orders, int(p.orders[0])
        self._initial_cache = None

    @classmethod
    def from_full_scale(cls, xp_rows, fp_rows, sections_rows, n: int, full_scale, **kw):
        """the stage whose gain[r] = hi / full_scale[r], so that a filtered +-full scale (volts) maps to +-hi (a scalar:
        every row).  ValueError: a full scale that is not finite or not positive."""
        return cls(xp_rows, fp_rows, sections_rows, n, _full_scale_gain('CurveIirDacStage', full_scale, kw), **kw)

    def kernel_name(self) -> str:
        """'iir_rows_curve_dac<T,NSEC,ORD>'"""
        return self.plan.kernel_name()

    def row_state(self, z, r: int):
        """row r's own state (scipy layout, its sections back to back) out of a (batch, state_dim) host array"""
        return _row_state(z, r, self.own_orders, self.section_order)

    def apply_torch(self, x, codes=None, counts=None, beyond=None, initial=0.0, zi=None, zf=None):
        """x: (batch, >= n) row-contiguous device tensor of the stage's dtype -- or ONE row, (1, >= n) or 1-D, that
        every row reads through its own curve and cascade (the shared-input form); codes: (batch, >= n) int16 (rows
        may be windows of a wider tensor; None: allocated); counts / beyond: None or contiguous (batch, 3) int64 device
        tensors, overwritten with the converter's / the curve's [below, above, nan]; `initial`: a scalar, one value
        per row, or a (batch,) float64 device tensor -- levels of the curve's OUTPUT; zi / zf: optional (batch,
        state_dim) float64 device tensors.  Out of place: `codes` may share no memory with `x`, a report with neither
        nor with the other report (ValueError); `x` is never written.  One kernel on torch's current stream, nothing
        else: no memset, allocation or synchronisation (with `codes` given and `initial` a scalar or a tensor).
        -> codes[:, :n]"""
        import torch
        if x.dim() == 1:
            x = x.unsqueeze(0)
        shared = self.batch > 1 and x.shape[0] == 1
        in_rows = 1 if shared else self.batch
        x0, xs = _rows.check_rows(x, in_rows, self.n, _rows.torch_dtype(self.dtype),
                                  'expected x: (batch, >=n) row-contiguous device tensor of the stage dtype, or one row')
        if codes is None:
            codes = torch.empty((self.batch, self.n), dtype=torch.int16, device=x.device)
        y0, ys = _rows.check_rows(codes, self.batch, self.n, torch.int16,
                                  'expected codes: (batch, >=n) row-contiguous int16 device tensor')
        sides = (x0, xs, in_rows, self.n, self.dtype.itemsize), (y0, ys, self.batch, self.n, 2)
        c0, b0, zip_, zfp = _check_reports('curve iir dac stage', 'codes', 'batch', self.batch, sides, counts, beyond,
                                           zi, zf, self.state_dim)
        ini = _initial_rows(self, self.batch, initial, x.device)
        inip = None if ini is None else ini.data_ptr()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if shared:
            self.plan.apply_shared_in(x0, y0, ys, c0, b0, zip_, zfp, inip, stream)
        else:
            self.plan.apply(x0, xs, y0, ys, c0, b0, zip_, zfp, inip, stream)
        return codes[:, :self.n]

    def close(self):
        self.plan.close()


def curve_iir_dac_rows(sig, xp_rows, fp_rows, filters_rows, gain, offset=0.0, bits=16, shift=0, left=None, right=None,
                       initial=0.0, return_counts=False):
    """`iir_dac_rows(interp_rows(sig, xp_rows, fp_rows, left, right), filters_rows, gain, offset, bits, shift, initial)`
    in one launch (see `CurveIirDacStage`): NumPy in, NumPy out, (rows, samples) int16.  `xp_rows` / `fp_rows`: one
    curve per row, or one 1-D pair for every row; `filters_rows`: one list of (b, a) sections per row; `initial`: a
    scalar or one level (of the curve's output) per row.  float32 rows stay float32 on the way in, anything else is read
    as float64.  `return_counts`: -> (codes, counts, beyond), the converter's and the curve's (rows, 3) int64 [below,
    above, nan].  ValueError before any device work: sig not 2-D, what `CurveIirDacStage` refuses.
    NotImplementedError: complex rows, curves or coefficients."""
    sig2 = _rows_signal_f32('curve_iir_dac_rows', sig)
    batch, n = sig2.shape
    _engine.curve_rows_arguments(xp_rows, fp_rows, left, right, batch, n, sig2.dtype)          # the curve's rules first
    filters_rows = [list(f) for f in filters_rows]
    gains = _per_row('curve_iir_dac_rows', 'gain', gain, batch)
    offsets = _per_row('curve_iir_dac_rows', 'offset', offset, batch)
    _engine.dac_rows_arguments(gains, offsets, n, bits, shift, 1, sig2.dtype)
    if len(filters_rows) != batch:
        raise ValueError(f'curve_iir_dac_rows: {len(filters_rows)} filter lists for {batch} rows')
    packed = _engine.pack_sections_rows(filters_rows)
    ini = _initial_host(initial, batch, 'curve_iir_dac_rows: initial is a scalar or one value per row')
    return _one_shot(
        sig2, lambda: _engine.CurveIirDacPlan(xp_rows, fp_rows, filters_rows, gains, offsets, n, bits, shift, left, right,
                                              batch, sig2.dtype, packed=packed),
        lambda plan, x, y, reports, levels: plan.apply(x, n, y, n, reports[0], reports[1], None, None, levels),
        shape=(batch, n), dtype=np.int16, report_rows=batch, reports=2, return_counts=return_counts, initial=ini)


class SampledCurveIirDac(_LentScratch):
    """`BatchSampler(channels, grid)` (float64 rows), `CurveStage(xp_rows, fp_rows, n, left=, right=)` in place and
    `IirDacStage(filters_rows, n, gain, offset, bits, shift)`, device-resident and bit for bit -- codes, both reports
    and zf -- with the float64 rows left out: a whole flux line programmed in its physical unit -- waveform, measured
    curve to volts, exp-decay correction, converter -- in ONE kernel with 2 B per sample of HBM traffic.  `fused`
    exactly where `SampledIirDac` is (same decision, same `why_not` texts), but for curves whose knots do not fit next
    to the fine-grid fill's LDS (more than 567 knots in a row there): `kernel_name()` is
    'iir_rows_sampled_curve_dac<f64,NSEC,ORD>' on fine grids, 'iir_rows_short_curve_dac<f64,NSEC,ORD>' at AWG sample
    rates, and every sample the fill produces goes through the row's curve before it enters the filter.  Plans that do
    not fuse run the sampler into a float64 scratch taken once, here, and then 'iir_rows_curve_dac<f64,NSEC,ORD>': two
    launches and 18 B per sample instead of three and 34.  float64 only; complex rows are refused.  The curves follow
    `CurveStage`'s rules (whoever measured f(V) passes `CurveStage.inverse_rows(volts, detuning)`), the cascades
    `IirStage`'s per-row rules, gain / offset / bits / shift `DacStage`'s; a refusal names the curve first, then the
    converter, then the cascade.  `counts` is the converter's [below, above, nan] per channel, `beyond` the curve's;
    `initial` holds levels of the curve's output (volts).  Build once, launch many times.  It saves the float64 rows and
    two launches, not time: as measured the three launches are faster.

        sd = SampledCurveIirDac.from_full_scale(channels, wl.awg_grid(n, 2e9), xs, fs, filters_rows, 1.0)
        sd.launch_torch(codes, counts=clipped, beyond=outside, initial=levels, zf=zf)
    """

    def __init__(self, channels, grid, xp_rows, fp_rows, filters_rows, gain, offset=0.0, bits: int = 16, shift: int = 0,
                 left=None, right=None, function_lib=None, tile=1):
        """`tile` > 1 repeats the channel list that many times (synthetic batches, as BatchSampler's)"""
        from . import _flatten
        channels, filters_rows = list(channels), list(filters_rows)
        rows = len(channels) * max(int(tile), 1)
        if rows < 1:
            raise ValueError('SampledCurveIirDac: no rows')
        if not isinstance(grid, _flatten.wfk_grid):
            grid = _flatten.grid_from_desc(grid)
        # argument errors before any device work: the curve's, the converter's, the cascades'
        _engine.curve_rows_arguments(xp_rows, fp_rows, left, right, rows, int(grid.n), np.float64)
        gains, offsets = _gain_offset_rows('SampledCurveIirDac', gain, offset, rows)
        _engine.dac_rows_arguments(gains, offsets, int(grid.n), bits, shift, 1)
        if len(filters_rows) != rows:
            raise ValueError(f'SampledCurveIirDac: {len(filters_rows)} cascades for {rows} rows')
        packed = _engine.pack_sections_rows(filters_rows)
        self.prog = _flatten.tile_program(_flatten.flatten(channels, grid, function_lib), tile)
        if self.prog.n_channels != rows:
            raise ValueError(f'SampledCurveIirDac: {rows} cascades for {self.prog.n_channels} rows')
        if self.prog.complex_amp or self.prog.host_complex:
            raise NotImplementedError('complex rows')
        self.plan = _engine.ChainCurveIirDacPlan(self.prog, grid, xp_rows, fp_rows, filters_rows, gains, offsets, bits,
                                                 shift, left, right, packed=packed)
        p = self.plan
        self.n, self.n_channels, self.gain, self.offset = p.n, p.n_channels, p.gain, p.offset
        self.knots, self.left, self.right = p.knots, p.left, p.right
        self.bits, self.shift, self.lo, self.hi = p.bits, p.shift, p.lo, p.hi
        self.state_dim, self.own_orders, self.section_order = p.state_dim, packed[3], int(packed[0][0])
        self.fused, self.why_not = p.fused, p.why_not
        self._initial_cache = None
        self._take_scratch()                                       # the unfused path's float64 rows: taken once, here

    @classmethod
    def from_full_scale(cls, channels, grid, xp_rows, fp_rows, filters_rows, full_scale, **kw):
        """the plan whose gain[r] = hi / full_scale[r], so that a filtered +-full scale (volts) maps to +-hi (a scalar:
        every row).  ValueError: a full scale that is not finite or not positive."""
        return cls(channels, grid, xp_rows, fp_rows, filters_rows,
                   _full_scale_gain('SampledCurveIirDac', full_scale, kw), **kw)

    def row_state(self, z, r: int):
        """row r's own state (scipy layout, its sections back to back) out of a (n_channels, state_dim) host array"""
        return _row_state(z, r, self.own_orders, self.section_order)

    def kernel_name(self) -> str:
        """'iir_rows_sampled_curve_dac<f64,NSEC,ORD>' | 'iir_rows_short_curve_dac<f64,NSEC,ORD>' | '<sampler kernels> +
        iir_rows_curve_dac<f64,NSEC,ORD>'"""
        return self.plan.kernel_name()

    def launch(self, out_ptr, out_stride=None, counts_ptr=None, beyond_ptr=None, zi_ptr=None, zf_ptr=None,
               initial_ptr=None, stream=0):
        """raw pointers; out_stride in codes (None: n); initial_ptr: device array of n_channels doubles or None"""
        s = self._scratch
        self.plan.launch(out_ptr, self.n if out_stride is None else out_stride, counts_ptr, beyond_ptr,
                         None if s is None else s.ptr, self.n, zi_ptr, zf_ptr, initial_ptr, stream)

    def launch_torch(self, codes, counts=None, beyond=None, initial=0.0, zi=None, zf=None):
        """codes: (n_channels, >= n) row-contiguous int16 device tensor (rows may be a window of a wider tensor);
        counts / beyond: None or contiguous (n_channels, 3) int64 device tensors, overwritten with the converter's /
        the curve's [below, above, nan] per channel; a report may share no memory with `codes` or with the other
        (ValueError); `initial`: a scalar, one value per row, or a (n_channels,) float64 device tensor; zi / zf:
        optional (n_channels, state_dim) float64 device tensors.  Asynchronous on torch's current stream: one kernel
        (two where not `fused`), no memset, allocation or synchronisation.  -> codes[:, :n]"""
        import torch
        y0, ys = _rows.check_rows(codes, self.n_channels, self.n, torch.int16,
                                  'expected codes: (n_channels, >=n) row-contiguous int16 device tensor')
        c0, b0, zip_, zfp = _check_reports('sampled curve iir dac', 'codes', 'n_channels', self.n_channels,
                                           ((y0, ys, self.n_channels, self.n, 2), ), counts, beyond,
                                           zi, zf, self.state_dim)
        ini = _initial_rows(self, self.n_channels, initial, codes.device)
        self.launch(y0, ys, c0, b0, zip_, zfp, None if ini is None else ini.data_ptr(),
                    torch.cuda.current_stream(codes.device).cuda_stream)
        return codes[:, :self.n]

    def to_host(self, initial=0.0, zi=None, return_counts=False, return_beyond=False, return_zf=False):
        """NumPy codes (n_channels, n) [, counts (n_channels, 3)] [, beyond (n_channels, 3)] [, zf (n_channels,
        state_dim)]; initial: a scalar or one value per row; zi: (n_channels, state_dim)"""
        return _host_trip(
            lambda y, reports, dzi, dzf, levels: self.launch(y, None, reports[0], reports[1], dzi, dzf, levels),
            shape=(self.n_channels, self.n), dtype=np.int16, rows=self.n_channels,
            reports=(return_counts, return_beyond), state_dim=self.state_dim, zi=zi, return_zf=return_zf, initial=initial)


class MarkerStage:
    """Device-resident gate markers for `batch` rows of `n` samples (build once, apply many times): the marker line
    that opens a switch or blanks an amplifier around every pulse, from the IDEAL gate rows (exact zeros outside the
    pulses, as the sampler writes them), into the bit `DacStage(shift=...)` left free.  `group` = k in {1, 2} input
    rows drive one marker row (k = 2: the I and Q of a pair, as `DacStage(interleave=2)` pairs them);
    `.out_rows = batch // group`.  Exact, in integers:
        active[g, i] = any_j |x[g k + j, i]| > threshold[g]         (NaN inactive, +-inf active)
        m[g, i]      = any active[g, j], j in [i - trail[g], i + lead[g]], clipped to the row
    so a marker rises `lead` samples before a burst and falls `trail` samples after it, and gaps shorter than
    lead + trail + 1 close.  `lead` / `trail` (samples, 0 .. 4096) / `threshold` (>= 0): a scalar (every marker row;
    give `batch`, the number of INPUT rows) or one value per marker row.  An optional (out_rows, 2) int64 counts
    tensor is OVERWRITTEN by every apply with [high, pulses] per marker row: the samples with m = 1 and its rising
    edges (a marker high at i = 0 counts).

        mk = MarkerStage(n, lead=20, trail=10, group=2, batch=rows)
        mk.apply_codes_torch(gates, codes, bit=0)               # in place in the codes, on torch's current stream
    """

    _X_ROWS = 'expected x: (batch, >=n) row-contiguous device tensor of the stage dtype'

    def __init__(self, n: int, lead=0, trail=0, threshold=0.0, group: int = 1, dtype=np.float64, batch=None):
        group = int(group)
        if group not in (1, 2):
            raise ValueError('MarkerStage: group must be 1 or 2')
        given = [np.size(v) for v in (lead, trail, threshold) if np.ndim(v) > 0]
        if batch is None:
            if not given:
                raise ValueError('MarkerStage: scalar lead, trail and threshold need batch=')
            batch = given[0] * group
        batch = int(batch)
        if batch < 1:
            raise ValueError('MarkerStage: no rows')
        if batch % group:
            raise ValueError(f'MarkerStage: {batch} rows are no multiple of the group {group}')
        leads, trails, thresholds = (_per_row_flat('MarkerStage', what, v, batch // group)
                                     for what, v in (('lead', lead), ('trail', trail), ('threshold', threshold)))
        self.plan = _engine.MarkerRowsPlan(thresholds, leads, trails, n, group, dtype)
        p = self.plan
        self.n, self.batch, self.group, self.out_rows, self.dtype = p.n, p.batch, p.group, p.out_rows, p.dtype
        self.lead, self.trail, self.threshold = p.lead, p.trail, p.threshold

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, stream=0):
        self.plan.apply(in_ptr, in_stride, out_ptr, out_stride, counts_ptr, stream)

    def apply_codes(self, in_ptr, in_stride, codes_ptr, codes_stride, bit=0, counts_ptr=None, stream=0):
        self.plan.apply_codes(in_ptr, in_stride, codes_ptr, codes_stride, bit, counts_ptr, stream)

    def span(self, codes: bool = False) -> int:
        """the samples one workgroup covers: as bytes, or (`codes`) into codes"""
        return self.plan.span(codes)

    def kernel_name(self, codes: bool = False, counts: bool = False) -> str:
        return self.plan.kernel_name(codes, counts)

    def _checked(self, x, out, out_n, out_dtype, what, counts):
        """the row rule of both torch calls -> (x ptr, x stride, out ptr, out stride, counts ptr or None)"""
        x0, xs = _rows.check_rows(x, self.batch, self.n, _rows.torch_dtype(self.dtype), self._X_ROWS)
        y0, ys = _rows.check_rows(out, self.out_rows, out_n, _rows.torch_dtype(out_dtype),
                                  f'expected {what}: (out_rows, >={"group * " if out_dtype == np.int16 else ""}n) '
                                  f'row-contiguous {np.dtype(out_dtype).name} device tensor')
        c0 = _rows.check_state(counts, (self.out_rows, 2),
                               'expected counts: contiguous (out_rows, 2) int64 device tensor', dtype=np.int64)
        xr = (x0, xs, self.batch, self.n, self.dtype.itemsize)
        yr = (y0, ys, self.out_rows, out_n, np.dtype(out_dtype).itemsize)
        if not _rows.rows_disjoint(xr, yr):
            raise ValueError(f'marker stage: {what} overlaps x')
        if not _rows.report_disjoint(c0, self.out_rows, 2, xr, yr):
            raise ValueError(f'marker stage: counts overlaps x / {what}')
        return x0, xs, y0, ys, c0

    def apply_torch(self, x, out=None, counts=None):
        """x: (batch, >= n) row-contiguous device tensor of the stage's dtype; out: (out_rows, >= n) uint8 (rows may
        be windows of a wider tensor; None: allocated); counts: None or a contiguous (out_rows, 2) int64 device
        tensor, overwritten.  `out` may share no memory with `x`, `counts` with neither (ValueError); `x` is never
        written.  Asynchronous on torch's current stream.  -> out[:, :n]"""
        import torch
        if out is None:
            _rows.check_rows(x, self.batch, self.n, _rows.torch_dtype(self.dtype), self._X_ROWS)
            out = torch.empty((self.out_rows, self.n), dtype=torch.uint8, device=x.device)
        x0, xs, y0, ys, c0 = self._checked(x, out, self.n, np.uint8, 'out', counts)
        self.apply(x0, xs, y0, ys, c0, torch.cuda.current_stream(x.device).cuda_stream)
        return out[:, :self.n]

    def apply_codes_torch(self, x, codes, bit: int = 0, counts=None):
        """x as in `apply_torch`; codes: (out_rows, >= group * n) row-contiguous int16 device tensor in the layout
        `DacStage(interleave=group)` writes, changed IN PLACE: bit `bit` (0 .. 15) of every code becomes the marker
        of its sample -- overwritten, not OR-ed -- and no other bit changes.  -> codes[:, :group * n]"""
        import torch
        if not 0 <= int(bit) <= 15:
            raise ValueError('bit must lie in [0, 15]')
        x0, xs, y0, ys, c0 = self._checked(x, codes, self.group * self.n, np.int16, 'codes', counts)
        self.apply_codes(x0, xs, y0, ys, int(bit), c0, torch.cuda.current_stream(x.device).cuda_stream)
        return codes[:, :self.group * self.n]

    def close(self):
        self.plan.close()


def marker_rows(sig, lead=0, trail=0, threshold=0.0, group=1, codes=None, bit=0, return_counts=False):
    """The gate markers of a 2-D real `sig` (see `MarkerStage` for the formula), all rows in one launch: NumPy in,
    NumPy out.  -> uint8 (rows // group, samples); with `codes` ((rows // group, group * samples) int16, the layout of
    `dac_codes_rows(interleave=group)`): a COPY of them with bit `bit` of every code replaced by the marker of its
    sample.  `lead` / `trail` / `threshold`: a scalar (every marker row) or one value per marker row.  float32 rows
    stay float32 on the way in, anything else is read as float64.  `return_counts`: -> (result, counts), counts the
    (rows // group, 2) int64 [high, pulses] per marker row.  ValueError before any device work: sig not 2-D, a number
    of leads, trails or thresholds that does not match, codes of another shape or dtype, a bit outside 0 .. 15, what
    `MarkerStage` refuses.  NotImplementedError: complex rows."""
    sig2 = _rows_signal_f32('marker_rows', sig)
    batch, n = sig2.shape
    group = int(group)
    if group not in (1, 2):
        raise ValueError('marker_rows: group must be 1 or 2')
    if batch < 1:
        raise ValueError('marker_rows: no rows')
    if batch % group:
        raise ValueError(f'marker_rows: {batch} rows are no multiple of the group {group}')
    rows = batch // group
    leads, trails, thresholds = (_per_row('marker_rows', what, v, rows)
                                 for what, v in (('lead', lead), ('trail', trail), ('threshold', threshold)))
    th, le, tr, n, group, dtype = _engine.marker_rows_arguments(thresholds, leads, trails, n, group, sig2.dtype)
    if not 0 <= int(bit) <= 15:
        raise ValueError('marker_rows: bit must lie in [0, 15]')
    if codes is not None:
        codes = np.asarray(codes)
        if codes.dtype != np.int16 or codes.shape != (rows, group * n):
            raise ValueError(f'marker_rows: codes must be int16 of shape ({rows}, {group * n})')
        codes = np.ascontiguousarray(codes)
    if n == 0:
        res = codes.copy() if codes is not None else np.zeros((rows, 0), dtype=np.uint8)
        return (res, np.zeros((rows, 2), dtype=np.int64)) if return_counts else res
    out_bytes = codes.nbytes if codes is not None else rows * n
    with _engine.MarkerRowsPlan(th, le, tr, n, group, dtype) as plan, _engine.DeviceBuffer(sig2.nbytes) as x, \
            _engine.DeviceBuffer(out_bytes) as y, _engine.DeviceBuffer(rows * 16) as c:
        x.upload(sig2)
        if codes is not None:
            y.upload(codes)
            plan.apply_codes(x.ptr, n, y.ptr, group * n, int(bit), c.ptr if return_counts else None)
        else:
            plan.apply(x.ptr, n, y.ptr, n, c.ptr if return_counts else None)
        _engine.sync()
        res = y.download((rows, group * n), np.int16) if codes is not None else y.download((rows, n), np.uint8)
        return (res, c.download((rows, 2), np.int64)) if return_counts else res


class SegmentStage:
    """Device-resident cut of `batch` rows of `width` * n int16 DAC codes at their marker (build once, apply many
    times): what an AWG with a sequencer is programmed with -- a short table of (play this stretch, from here) and
    the kept samples packed back to back -- so that only the stretches around the pulses are downloaded.
    `width` = k in {1, 2} codes per sample (k = 2: the layout of `DacStage(interleave=2)` / `MarkerStage(group=2)`).
    The mask is, per apply, one bit of the codes (`bit=`: any of a sample's k codes) or a (batch, n) uint8 tensor as
    `MarkerStage.apply_torch` writes it (`marks=`).  `align` = A, a power of two in [1, 4096], is the instrument's
    granularity: granule q = samples [q A, min((q + 1) A, n)) is kept when any of them is marked; a segment is a
    maximal run [q0, q1) of kept granules, in ascending order:
        start = q0 A,   length = min(q1 A, n) - start,   offset = the lengths before it,   kept = all lengths.
    An apply writes `table` (batch, max_segments, 3) int32 [start, length, offset] for the first min(count,
    max_segments) segments of each row, `packed` (batch, width * capacity) int16, the codes of the first min(kept,
    capacity) kept samples verbatim, and `used` (batch, 2) int64 [count, kept] -- the TRUE totals, overwritten by
    every apply; nothing else of table and packed is touched.  `max_segments` defaults to ceil(ceil(n / A) / 2) and
    `capacity` to n, the sizes that cannot overflow.  Building a stage needs no device; the plan is made by the first
    apply and owns a workspace, so a stage serves one stream at a time.

        seg = SegmentStage(n, batch=rows, width=2, align=16)
        rows_out = seg.download(*seg.apply_torch(codes, bit=0))     # [(table_r, packed_r), ...]
    """

    def __init__(self, n: int, batch: int = 1, width: int = 1, align: int = 1, max_segments=None, capacity=None):
        try:
            (self.n, self.batch, self.width, self.align, self.max_segments,
             self.capacity) = _engine.segment_rows_arguments(n, batch, width, align, max_segments, capacity)
        except ValueError as e:
            raise ValueError(f'SegmentStage: {e}') from None
        self.plan = None

    def _plan(self):
        if self.plan is None:
            self.plan = _engine.SegmentRowsPlan(self.n, self.batch, self.width, self.align, self.max_segments,
                                                self.capacity)
        return self.plan

    def span(self) -> int:
        """the samples one workgroup covers"""
        return self._plan().span()

    def kernel_name(self, launch: int = 0, marks: bool = False) -> str:
        return self._plan().kernel_name(launch, marks)

    def _inputs(self, codes, bit, marks):
        """-> (sides of the inputs as _rows.rows_disjoint takes them, codes ptr, stride, marks ptr or None, stride)"""
        if (bit is None) == (marks is None):
            raise ValueError('segment stage: give exactly one of bit= and marks=')
        if bit is not None and not 0 <= int(bit) <= 15:
            raise ValueError('segment stage: bit must lie in [0, 15]')
        k = self.width
        c0, cs = _rows.check_rows(codes, self.batch, k * self.n, _rows.torch_dtype(np.int16),
                                  'expected codes: (batch, >=width * n) row-contiguous int16 device tensor')
        sides = [(c0, cs, self.batch, k * self.n, 2)]
        m0 = ms = None
        if marks is not None:
            m0, ms = _rows.check_rows(marks, self.batch, self.n, _rows.torch_dtype(np.uint8),
                                      'expected marks: (batch, >=n) row-contiguous uint8 device tensor')
            sides.append((m0, ms, self.batch, self.n, 1))
        return sides, c0, cs, m0, ms

    def _used(self, used, sides):
        u0 = _rows.check_state(used, (self.batch, 2), 'expected used: contiguous (batch, 2) int64 device tensor',
                               dtype=np.int64)
        if not _rows.report_disjoint(u0, self.batch, 2, *sides):
            raise ValueError('segment stage: used overlaps codes / marks / table / packed')
        return u0

    def _launch(self, codes, bit, c0, cs, m0, ms, t0, ts, p0, ps, u0):
        import torch
        stream = torch.cuda.current_stream(codes.device).cuda_stream
        if bit is not None:
            self._plan().apply_bit(c0, cs, int(bit), t0, ts, p0, ps, u0, stream)
        else:
            self._plan().apply_marks(c0, cs, m0, ms, t0, ts, p0, ps, u0, stream)

    def apply_torch(self, codes, *, bit=None, marks=None, table=None, packed=None, used=None):
        """codes: (batch, >= width * n) row-contiguous int16 device tensor; exactly one of `bit` (0 .. 15) and `marks`
        ((batch, >= n) uint8); table: (batch, max_segments, 3) int32, rows may be windows of a wider tensor; packed:
        (batch, >= width * capacity) int16; used: contiguous (batch, 2) int64 -- each allocated when None.  No output
        may share memory with an input or another output (ValueError); codes and marks are never written.
        Asynchronous on torch's current stream, no allocation when the outputs are given.  -> (table, packed[:, :width
        * capacity], used)"""
        import torch
        k, rows = self.width, self.batch
        sides, c0, cs, m0, ms = self._inputs(codes, bit, marks)
        if table is None:
            table = torch.empty((rows, max(self.max_segments, 1), 3), dtype=torch.int32,
                                device=codes.device)[:, :self.max_segments]
        if packed is None:
            packed = torch.empty((rows, max(k * self.capacity, 1)), dtype=torch.int16,
                                 device=codes.device)[:, :k * self.capacity]
        if used is None:
            used = torch.empty((rows, 2), dtype=torch.int64, device=codes.device)
        width3 = 3 * self.max_segments
        if (table.dim() != 3 or tuple(table.shape) != (rows, self.max_segments, 3)
                or (self.max_segments > 1 and table.stride(1) != 3) or (self.max_segments > 0 and table.stride(2) != 1)):
            raise ValueError('expected table: (batch, max_segments, 3) int32 device tensor, each row contiguous')
        t0, ts = _rows.check_rows(table.as_strided((rows, width3), (table.stride(0), 1)), rows, width3,
                                  _rows.torch_dtype(np.int32),
                                  'expected table: (batch, max_segments, 3) int32 device tensor, each row contiguous')
        p0, ps = _rows.check_rows(packed, rows, k * self.capacity, _rows.torch_dtype(np.int16),
                                  'expected packed: (batch, >=width * capacity) row-contiguous int16 device tensor')
        tr, pr = (t0, ts, rows, width3, 4), (p0, ps, rows, k * self.capacity, 2)
        for s, what in zip(sides, ('codes', 'marks')):
            if not _rows.rows_disjoint(s, tr):
                raise ValueError(f'segment stage: table overlaps {what}')
            if not _rows.rows_disjoint(s, pr):
                raise ValueError(f'segment stage: packed overlaps {what}')
        if not _rows.rows_disjoint(tr, pr):
            raise ValueError('segment stage: table overlaps packed')
        u0 = self._used(used, sides + [tr, pr])
        # a side that holds nothing is not looked at; both: the sizing pass, which writes the same `used`
        self._launch(codes, bit, c0, cs, m0, ms, t0 if width3 else None, ts, p0 if self.capacity else None, ps, u0)
        return table, packed[:, :k * self.capacity], used

    def measure_torch(self, codes, *, bit=None, marks=None, used=None):
        """the sizing pass: only `used` (allocated when None) is written.  -> used"""
        import torch
        sides, c0, cs, m0, ms = self._inputs(codes, bit, marks)
        if used is None:
            used = torch.empty((self.batch, 2), dtype=torch.int64, device=codes.device)
        u0 = self._used(used, sides)
        self._launch(codes, bit, c0, cs, m0, ms, None, 0, None, 0, u0)
        return used

    def download(self, table, packed, used):
        """what an apply wrote, on the host: `used` is copied first (this waits for the stream), then only
        [:, :max count] of the table and [:, :width * max kept] of packed, through pinned host memory (torch's cache of
        it: the arrays returned are views of that memory and keep it alive).  -> a list of (table_r (count_r, 3) int32,
        packed_r (width * kept_r,) int16), one per row.  ValueError when a row overflowed max_segments or capacity:
        what came out would not be the row."""
        import torch

        def to_host(x):
            if x.numel() == 0:
                return np.empty(tuple(x.shape), dtype=x.cpu().numpy().dtype)
            h = torch.empty(tuple(x.shape), dtype=x.dtype, pin_memory=True)
            h.copy_(x, non_blocking=True)
            torch.cuda.current_stream(x.device).synchronize()
            return h.numpy()

        u = used.cpu().numpy()
        for r in range(self.batch):
            if u[r, 0] > self.max_segments or u[r, 1] > self.capacity:
                raise ValueError(f'segment stage: row {r} overflowed: {int(u[r, 0])} segments of {int(u[r, 1])} samples, '
                                 f'room for {self.max_segments} of {self.capacity}')
        k = self.width
        count, kept = (int(u[:, 0].max()), int(u[:, 1].max())) if self.batch else (0, 0)
        t, p = to_host(table[:, :count]), to_host(packed[:, :k * kept])
        return [(t[r, :int(u[r, 0])], p[r, :k * int(u[r, 1])]) for r in range(self.batch)]

    def close(self):
        if self.plan is not None:
            self.plan.close()
            self.plan = None


def segment_rows(codes, marks=None, bit=None, width=1, align=1):
    """The rows of a 2-D int16 `codes` ((rows, width * n)) cut at their marker (see `SegmentStage`), all rows in one
    apply with the sizes that cannot overflow: NumPy in, NumPy out.  Exactly one of `marks` ((rows, n), non-zero =
    marked) and `bit` (0 .. 15).  -> a list of (table_r (count_r, 3) int32 [start, length, offset], packed_r
    (width * kept_r,) int16), one per row.  ValueError before any device work: codes not 2-D int16, a row length that
    is no multiple of the width, marks of another shape, neither or both of marks and bit, a bit outside 0 .. 15, what
    `SegmentStage` refuses."""
    codes = np.asarray(codes)
    if codes.ndim != 2 or codes.dtype != np.int16:
        raise ValueError('segment_rows: codes must be a 2-D int16 array')
    if (bit is None) == (marks is None):
        raise ValueError('segment_rows: give exactly one of bit= and marks=')
    if width not in (1, 2):
        raise ValueError('segment_rows: width must be 1 or 2')
    rows, nk = codes.shape
    if nk % width:
        raise ValueError(f'segment_rows: rows of {nk} codes are no multiple of the width {width}')
    try:
        n, rows, k, align, max_segments, _ = _engine.segment_rows_arguments(nk // width, rows, width, align)
    except ValueError as e:
        raise ValueError(f'segment_rows: {e}') from None
    if bit is not None and not 0 <= int(bit) <= 15:
        raise ValueError('segment_rows: bit must lie in [0, 15]')
    if marks is not None:
        marks = np.asarray(marks)
        if marks.shape != (rows, n):
            raise ValueError(f'segment_rows: marks must have the shape ({rows}, {n})')
        marks = np.ascontiguousarray(marks != 0, dtype=np.uint8)
    if n == 0:
        return [(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int16)) for _ in range(rows)]
    codes = np.ascontiguousarray(codes)
    with _engine.SegmentRowsPlan(n, rows, k, align, max_segments, n) as plan, \
            _engine.DeviceBuffer(codes.nbytes) as x, _engine.DeviceBuffer(rows * n if marks is not None else 16) as m, \
            _engine.DeviceBuffer(rows * max_segments * 12) as t, _engine.DeviceBuffer(codes.nbytes) as y, \
            _engine.DeviceBuffer(rows * 16) as u:
        x.upload(codes)
        if marks is not None:
            m.upload(marks)
            plan.apply_marks(x.ptr, k * n, m.ptr, n, t.ptr, 3 * max_segments, y.ptr, k * n, u.ptr)
        else:
            plan.apply_bit(x.ptr, k * n, int(bit), t.ptr, 3 * max_segments, y.ptr, k * n, u.ptr)
        _engine.sync()
        used = u.download((rows, 2), np.int64)
        table = t.download((rows, max_segments, 3), np.int32)
        packed = y.download((rows, k * n), np.int16)
    return [(table[r, :int(used[r, 0])].copy(), packed[r, :k * int(used[r, 1])].copy()) for r in range(rows)]


def expand_segments(table_row, packed_row, n, idle, width=1):
    """The inverse of the cut, on the host: a row of `width` * n int16 codes filled with `idle` (one code, or one per
    code of a sample) with the segments of `table_row` ((count, 3) [start, length, offset]) laid back from
    `packed_row`.  What an upload is checked against.  ValueError: a width other than 1 or 2, a table of another shape,
    a segment outside the row or outside the packed codes."""
    n, k = int(n), int(width)
    if k not in (1, 2):
        raise ValueError('expand_segments: width must be 1 or 2')
    if n < 0:
        raise ValueError('expand_segments: n must not be negative')
    table = np.asarray(table_row)
    packed = np.asarray(packed_row)
    if table.ndim != 2 or table.shape[1] != 3 or table.dtype.kind not in 'iu':
        raise ValueError('expand_segments: the table must be (count, 3) integers')
    if packed.ndim != 1 or packed.dtype != np.int16:
        raise ValueError('expand_segments: the packed codes must be 1-D int16')
    idle = np.asarray(idle, dtype=np.int16).reshape(-1)
    if len(idle) not in (1, k):
        raise ValueError('expand_segments: idle is one code or one per code of a sample')
    out = np.tile(idle, n * k // len(idle)).astype(np.int16)
    for j, (start, length, offset) in enumerate(table.astype(np.int64).tolist()):
        if start < 0 or length < 0 or start + length > n:
            raise ValueError(f'expand_segments: segment {j} lies outside the row')
        if offset < 0 or k * (offset + length) > len(packed):
            raise ValueError(f'expand_segments: segment {j} lies outside the packed codes')
        out[k * start:k * (start + length)] = packed[k * offset:k * (offset + length)]
    return out


class SegmentLibrary:
    """Device-resident waveform library of what a `SegmentStage` wrote (build once, apply many times): the segments
    of a row whose codes are equal share one slot, so that the waveform memory and the download scale with the
    distinct pulses of a channel, not with the pulses played.  `batch`, `max_segments`, `capacity` and `width` are
    those of the stage (`SegmentLibrary.of(stage)` takes them from it); `lib_capacity` in [0, capacity], default
    capacity, is the room of a library row in samples.
    Two segments of a row are equal when their lengths and their `width` * length codes are equal verbatim, marker
    bits included; among equal segments the one with the lowest j is the first.  The firsts in ascending j are the
    row's slots u = 0, 1, ...:
        lib_offset_u = the lengths of the slots before u,   unique = the slots,   lib_kept = the lengths of all slots.
    An apply reads `table`, `packed` and `used` as the stage wrote them, never writes them, and writes `plays`
    (batch, max_segments, 3) int32, entry j < count [start_j, length_j, lib_offset of the slot of j] -- the layout of
    `table`, so `expand_segments(plays_r, library_r, n, idle, width)` is the round trip -- `slots` (batch,
    max_segments) int32, the slot u of segment j < count, `library` (batch, width * lib_capacity) int16, the codes of
    slot u at width * lib_offset_u for the samples p < min(lib_kept, lib_capacity) (the cut is by position; `plays`
    holds the true offsets whatever the cut), and `lib_used` (batch, 2) int64 [unique, lib_kept] -- the TRUE totals,
    overwritten by every apply; nothing else of plays, slots and library is touched.
    A row that cannot be read -- `used` with count outside [0, max_segments] or kept outside [0, capacity], an entry
    j < count with length <= 0, offset < 0 or offset + length > capacity -- gets lib_used = [-1, -1] and nothing else
    of it is written; the other rows are unaffected.  Every output is a pure function of the inputs.
    Building a library needs no device; the plan is made by the first apply (WFK_SEGLIB_HASH_BITS is read then) and
    owns a workspace, so a library serves one stream at a time.

        lib = SegmentLibrary.of(seg)
        rows_out = lib.download(*lib.apply_torch(table, packed, used), used)    # [(plays_r, slots_r, library_r), ...]
    """

    def __init__(self, batch: int = 1, max_segments: int = 0, capacity: int = 0, width: int = 1, lib_capacity=None):
        try:
            (self.batch, self.width, self.max_segments, self.capacity,
             self.lib_capacity) = _engine.segment_library_arguments(batch, width, max_segments, capacity, lib_capacity)
        except ValueError as e:
            raise ValueError(f'SegmentLibrary: {e}') from None
        self.plan = None

    @classmethod
    def of(cls, stage, lib_capacity=None):
        """the library of what `stage` (a SegmentStage) writes"""
        return cls(stage.batch, stage.max_segments, stage.capacity, stage.width, lib_capacity)

    def _plan(self):
        if self.plan is None:
            self.plan = _engine.SegmentLibraryPlan(self.batch, self.width, self.max_segments, self.capacity,
                                                   self.lib_capacity)
        return self.plan

    def kernel_name(self, launch: int = 0) -> str:
        return self._plan().kernel_name(launch)

    def _table_like(self, t, what):
        """(batch, max_segments, 3) int32, each row contiguous -> (ptr, stride, side)"""
        rows, ms = self.batch, self.max_segments
        message = f'expected {what}: (batch, max_segments, 3) int32 device tensor, each row contiguous'
        if (t.dim() != 3 or tuple(t.shape) != (rows, ms, 3) or (ms > 1 and t.stride(1) != 3)
                or (ms > 0 and t.stride(2) != 1)):
            raise ValueError(message)
        p0, ps = _rows.check_rows(t.as_strided((rows, 3 * ms), (t.stride(0), 1)), rows, 3 * ms,
                                  _rows.torch_dtype(np.int32), message)
        return p0, ps, (p0, ps, rows, 3 * ms, 4)

    def _inputs(self, table, packed, used):
        """-> (the sides of the inputs with their names, table ptr, stride, packed ptr, stride, used ptr)"""
        rows, k = self.batch, self.width
        t0, ts, tr = self._table_like(table, 'table')
        p0, ps = _rows.check_rows(packed, rows, k * self.capacity, _rows.torch_dtype(np.int16),
                                  'expected packed: (batch, >=width * capacity) row-contiguous int16 device tensor')
        u0 = _rows.check_state(used, (rows, 2), 'expected used: contiguous (batch, 2) int64 device tensor',
                               dtype=np.int64)
        if u0 is None:
            raise ValueError('expected used: contiguous (batch, 2) int64 device tensor')
        sides = [('table', tr), ('packed', (p0, ps, rows, k * self.capacity, 2)), ('used', (u0, 2, rows, 2, 8))]
        return sides, t0, ts, p0, ps, u0

    def _lib_used(self, lib_used, sides):
        r0 = _rows.check_state(lib_used, (self.batch, 2),
                               'expected lib_used: contiguous (batch, 2) int64 device tensor', dtype=np.int64)
        if not _rows.report_disjoint(r0, self.batch, 2, *(s for _, s in sides)):
            raise ValueError('segment library: lib_used overlaps table / packed / used / plays / slots / library')
        return r0

    def apply_torch(self, table, packed, used, *, plays=None, slots=None, library=None, lib_used=None):
        """table: (batch, max_segments, 3) int32, packed: (batch, >= width * capacity) int16, used: contiguous
        (batch, 2) int64, as `SegmentStage.apply_torch` returns them (rows may be windows of wider tensors); plays:
        (batch, max_segments, 3) int32; slots: (batch, >= max_segments) int32; library: (batch, >= width *
        lib_capacity) int16; lib_used: contiguous (batch, 2) int64 -- each allocated when None.  No output may share
        memory with an input or another output (ValueError); the inputs are never written.  Asynchronous on torch's
        current stream, no allocation when the outputs are given.  -> (plays, slots, library[:, :width *
        lib_capacity], lib_used)"""
        import torch
        k, rows, ms = self.width, self.batch, self.max_segments
        sides, t0, ts, p0, ps, u0 = self._inputs(table, packed, used)
        device = table.device
        if plays is None:
            plays = torch.empty((rows, max(ms, 1), 3), dtype=torch.int32, device=device)[:, :ms]
        if slots is None:
            slots = torch.empty((rows, max(ms, 1)), dtype=torch.int32, device=device)[:, :ms]
        if library is None:
            library = torch.empty((rows, max(k * self.lib_capacity, 1)), dtype=torch.int16,
                                  device=device)[:, :k * self.lib_capacity]
        if lib_used is None:
            lib_used = torch.empty((rows, 2), dtype=torch.int64, device=device)
        y0, ys, yr = self._table_like(plays, 'plays')
        s0, ss = _rows.check_rows(slots, rows, ms, _rows.torch_dtype(np.int32),
                                  'expected slots: (batch, >=max_segments) row-contiguous int32 device tensor')
        l0, ls = _rows.check_rows(library, rows, k * self.lib_capacity, _rows.torch_dtype(np.int16),
                                  'expected library: (batch, >=width * lib_capacity) row-contiguous int16 device tensor')
        outs = [('library', (l0, ls, rows, k * self.lib_capacity, 2)), ('plays', yr), ('slots', (s0, ss, rows, ms, 4))]
        for i, (name, side) in enumerate(outs):
            for other, o in sides + outs[:i]:
                if not _rows.rows_disjoint(side, o):
                    raise ValueError(f'segment library: {name} overlaps {other}')
        r0 = self._lib_used(lib_used, sides + outs)
        stream = torch.cuda.current_stream(device).cuda_stream
        self._plan().apply(t0 if ms else None, ts, p0 if self.capacity else None, ps, u0, y0 if ms else None, ys,
                           s0 if ms else None, ss, l0 if self.lib_capacity else None, ls, r0, stream)
        return plays, slots, library[:, :k * self.lib_capacity], lib_used

    def measure_torch(self, table, packed, used, lib_used=None):
        """the sizing pass: only `lib_used` (allocated when None) is written.  -> lib_used"""
        import torch
        sides, t0, ts, p0, ps, u0 = self._inputs(table, packed, used)
        if lib_used is None:
            lib_used = torch.empty((self.batch, 2), dtype=torch.int64, device=table.device)
        r0 = self._lib_used(lib_used, sides)
        stream = torch.cuda.current_stream(table.device).cuda_stream
        self._plan().apply(t0 if self.max_segments else None, ts, p0 if self.capacity else None, ps, u0, None, 0, None,
                           0, None, 0, r0, stream)
        return lib_used

    def download(self, plays, slots, library, lib_used, used):
        """what an apply wrote, on the host: `lib_used` and `used` are copied first (this waits for the stream), then
        only [:, :max count] of plays and slots and [:, :width * max lib_kept] of the library, through pinned host
        memory (torch's cache of it: the arrays returned are views of that memory and keep it alive).  -> a list of
        (plays_r (count_r, 3) int32, slots_r (count_r,) int32, library_r (width * lib_kept_r,) int16), one per row.
        ValueError when a row could not be read or its library overflowed lib_capacity: what came out would not be
        the row."""
        import torch

        def to_host(x):
            if x.numel() == 0:
                return np.empty(tuple(x.shape), dtype=x.cpu().numpy().dtype)
            h = torch.empty(tuple(x.shape), dtype=x.dtype, pin_memory=True)
            h.copy_(x, non_blocking=True)
            torch.cuda.current_stream(x.device).synchronize()
            return h.numpy()

        lu, u = lib_used.cpu().numpy(), used.cpu().numpy()
        for r in range(self.batch):
            if lu[r, 0] < 0:
                raise ValueError(f'segment library: row {r} could not be read: its table, packed codes and totals do '
                                 f'not fit max_segments {self.max_segments} and capacity {self.capacity}')
            if lu[r, 1] > self.lib_capacity:
                raise ValueError(f'segment library: row {r} overflowed: {int(lu[r, 0])} slots of {int(lu[r, 1])} '
                                 f'samples, room for {self.lib_capacity}')
        k = self.width
        count, kept = (int(u[:, 0].max()), int(lu[:, 1].max())) if self.batch else (0, 0)
        p, s, y = to_host(plays[:, :count]), to_host(slots[:, :count]), to_host(library[:, :k * kept])
        return [(p[r, :int(u[r, 0])], s[r, :int(u[r, 0])], y[r, :k * int(lu[r, 1])]) for r in range(self.batch)]

    def close(self):
        if self.plan is not None:
            self.plan.close()
            self.plan = None


def library_rows(segments, width=1):
    """The waveform libraries of the rows that `segment_rows` returned (see `SegmentLibrary`), all rows in one apply:
    NumPy in, NumPy out.  `segments`: a list of (table_r (count_r, 3) int32, packed_r (width * kept_r,) int16), one
    per row.  -> a list of (plays_r (count_r, 3) int32, slots_r (count_r,) int32, library_r (width * lib_kept_r,)
    int16).  ValueError before any device work: no rows, a width other than 1 or 2, a table that is not (count, 3)
    int32, packed codes that are not 1-D int16 or no multiple of the width; ValueError after it: a row whose table
    does not fit its packed codes."""
    if width not in (1, 2):
        raise ValueError('library_rows: width must be 1 or 2')
    k = int(width)
    try:
        segments = [(np.asarray(t), np.asarray(p)) for t, p in segments]
    except (TypeError, ValueError):
        raise ValueError('library_rows: segments must be a list of (table, packed) pairs') from None
    rows = len(segments)
    if rows < 1:
        raise ValueError('library_rows: no rows')
    for r, (t, p) in enumerate(segments):
        if t.ndim != 2 or t.shape[1] != 3 or t.dtype != np.int32:
            raise ValueError(f'library_rows: row {r}: the table must be (count, 3) int32')
        if p.ndim != 1 or p.dtype != np.int16 or len(p) % k:
            raise ValueError(f'library_rows: row {r}: the packed codes must be 1-D int16, a multiple of the width long')
    ms, cap = max(len(t) for t, _ in segments), max(len(p) for _, p in segments) // k
    empty = [(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int16))
             for _ in range(rows)]
    if ms == 0:
        return empty
    try:
        _engine.segment_library_arguments(rows, k, ms, cap)
    except ValueError as e:
        raise ValueError(f'library_rows: {e}') from None
    table = np.zeros((rows, ms, 3), dtype=np.int32)
    packed = np.zeros((rows, max(k * cap, 1)), dtype=np.int16)
    used = np.zeros((rows, 2), dtype=np.int64)
    for r, (t, p) in enumerate(segments):
        table[r, :len(t)] = t
        packed[r, :len(p)] = p
        used[r] = len(t), len(p) // k
    with _engine.SegmentLibraryPlan(rows, k, ms, cap) as plan, _engine.DeviceBuffer(table.nbytes) as t, \
            _engine.DeviceBuffer(packed.nbytes) as y, _engine.DeviceBuffer(used.nbytes) as u, \
            _engine.DeviceBuffer(table.nbytes) as pl, _engine.DeviceBuffer(rows * ms * 4) as sl, \
            _engine.DeviceBuffer(packed.nbytes) as lb, _engine.DeviceBuffer(rows * 16) as lu:
        t.upload(table)
        y.upload(packed)
        u.upload(used)
        plan.apply(t.ptr, 3 * ms, y.ptr if cap else None, packed.shape[1], u.ptr, pl.ptr, 3 * ms, sl.ptr, ms,
                   lb.ptr if cap else None, packed.shape[1], lu.ptr)
        _engine.sync()
        lib_used = lu.download((rows, 2), np.int64)
        plays = pl.download((rows, ms, 3), np.int32)
        slots = sl.download((rows, ms), np.int32)
        library = lb.download(packed.shape, np.int16)
    for r in range(rows):
        if lib_used[r, 0] < 0:
            raise ValueError(f'library_rows: row {r}: the table does not fit the packed codes')
    return [(plays[r, :len(segments[r][0])].copy(), slots[r, :len(segments[r][0])].copy(),
             library[r, :k * int(lib_used[r, 1])].copy()) for r in range(rows)]


class SegmentPlayer:
    """Device-resident playback of a segment table (build once, apply many times): the inverse of the cut, what a
    sequencer plays from a table and a waveform memory, as `batch` dense rows of `width` * n int16 codes -- with an
    optional comparison against the rows the table was cut from, in the same pass.  `max_segments` and `capacity` (the
    room of a packed / library row, in samples) are those of the tensors it is given: `SegmentPlayer.of(stage)` takes
    them from a `SegmentStage`, `SegmentPlayer.of(library, n)` from a `SegmentLibrary` (capacity = its lib_capacity).
    An apply reads `table` (batch, max_segments, 3) int32 [start, length, offset] -- the stage's `table`, the
    library's `plays`, or one the user wrote --, `packed` (batch, >= width * capacity) int16 and `used` (batch, 2)
    int64, of which only the count of a row is read, and never writes them.  A row is GOOD when 0 <= count <=
    max_segments, every entry j < count has length > 0, start >= 0, start + length <= n, offset >= 0 and offset +
    length <= capacity, and every entry after the first starts at or after the end of the one before: ascending and
    disjoint.  Everything the two stages write is good; a table that overflowed max_segments, or a library cut at
    lib_capacity, is not.  This is NARROWER than `expand_segments`, which takes empty and overlapping entries (the
    later one wins).  For a good row, sample i of `out` holds the `width` codes at width * (offset_j + i - start_j) of
    packed where start_j <= i < start_j + length_j, and `idle` (one code, or one per code of a sample; passed by value,
    so a captured graph replays the captured codes) elsewhere: `expand_segments(table_r[:count], packed_r, n, idle,
    width)`, bit for bit.  All width * n codes of a good row are written and nothing else.  `report` (batch, 4) int64 is
    [played, differ, stray, first] per row, overwritten by every apply: played = the lengths of the entries; differ =
    the samples inside a play where any code differs from `expect`; stray = the samples outside every play where any
    code of `expect` differs from its idle -- what the cut threw away; first = the lowest sample counted by either, or
    -1; without `expect` [played, 0, 0, -1].  A bad row gets [-1, -1, -1, -1], nothing of its `out` is written, and the
    other rows are unaffected.  Building a player needs no device; the plan is made by the first apply and owns a
    workspace, so a player serves one stream at a time.

        player = SegmentPlayer.of(seg)
        played, report = player.apply_torch(table, packed, used, idle=idle, expect=codes)
    """

    def __init__(self, n: int, batch: int = 1, width: int = 1, max_segments: int = 0, capacity: int = 0):
        try:
            (self.n, self.batch, self.width, self.max_segments,
             self.capacity) = _engine.segment_play_arguments(n, batch, width, max_segments, capacity)
        except ValueError as e:
            raise ValueError(f'SegmentPlayer: {e}') from None
        self.plan = None

    @classmethod
    def of(cls, source, n=None):
        """the player of what `source` writes: a SegmentStage (its table / packed; n is the stage's), or a
        SegmentLibrary with the rows' n (its plays / library)"""
        if isinstance(source, SegmentStage):
            if n is not None and int(n) != source.n:
                raise ValueError(f'SegmentPlayer: n = {n} is not the n of the stage, {source.n}')
            return cls(source.n, source.batch, source.width, source.max_segments, source.capacity)
        if isinstance(source, SegmentLibrary):
            if n is None:
                raise ValueError('SegmentPlayer: a SegmentLibrary does not know n: give SegmentPlayer.of(library, n)')
            return cls(n, source.batch, source.width, source.max_segments, source.lib_capacity)
        raise ValueError('SegmentPlayer: of() takes a SegmentStage or a SegmentLibrary')

    def _plan(self):
        if self.plan is None:
            self.plan = _engine.SegmentPlayPlan(self.n, self.batch, self.width, self.max_segments, self.capacity)
        return self.plan

    def span(self) -> int:
        """the samples one workgroup of the second launch covers"""
        return self._plan().span()

    def kernel_name(self, launch: int = 0) -> str:
        return self._plan().kernel_name(launch)

    def _inputs(self, table, packed, used, expect):
        """-> (the sides of the inputs with their names, table ptr, stride, packed ptr, stride, used ptr, expect ptr
        or None, stride)"""
        rows, k, ms = self.batch, self.width, self.max_segments
        message = 'expected table: (batch, max_segments, 3) int32 device tensor, each row contiguous'
        if (table.dim() != 3 or tuple(table.shape) != (rows, ms, 3) or (ms > 1 and table.stride(1) != 3)
                or (ms > 0 and table.stride(2) != 1)):
            raise ValueError(message)
        t0, ts = _rows.check_rows(table.as_strided((rows, 3 * ms), (table.stride(0), 1)), rows, 3 * ms,
                                  _rows.torch_dtype(np.int32), message)
        p0, ps = _rows.check_rows(packed, rows, k * self.capacity, _rows.torch_dtype(np.int16),
                                  'expected packed: (batch, >=width * capacity) row-contiguous int16 device tensor')
        u0 = _rows.check_state(used, (rows, 2), 'expected used: contiguous (batch, 2) int64 device tensor',
                               dtype=np.int64)
        if u0 is None:
            raise ValueError('expected used: contiguous (batch, 2) int64 device tensor')
        sides = [('table', (t0, ts, rows, 3 * ms, 4)), ('packed', (p0, ps, rows, k * self.capacity, 2)),
                 ('used', (u0, 2, rows, 2, 8))]
        e0 = es = None
        if expect is not None:
            e0, es = _rows.check_rows(expect, rows, k * self.n, _rows.torch_dtype(np.int16),
                                      'expected expect: (batch, >=width * n) row-contiguous int16 device tensor')
            sides.append(('expect', (e0, es, rows, k * self.n, 2)))
        return sides, t0, ts, p0, ps, u0, e0, es

    def _report(self, report, sides, device):
        import torch
        if report is None:
            report = torch.empty((self.batch, 4), dtype=torch.int64, device=device)
        r0 = _rows.check_state(report, (self.batch, 4), 'expected report: contiguous (batch, 4) int64 device tensor',
                               dtype=np.int64)
        if not _rows.report_disjoint(r0, self.batch, 4, *(s for _, s in sides)):
            raise ValueError('segment play: report overlaps table / packed / used / expect / out')
        return report, r0

    def _launch(self, device, t0, ts, p0, ps, u0, idle, o0, os_, e0, es, r0):
        import torch
        ms, cap, n = self.max_segments, self.capacity, self.n
        self._plan().apply(t0 if ms else None, ts, p0 if cap else None, ps, u0, idle, o0 if n else None, os_ or 0,
                           e0 if n else None, es or 0, r0, torch.cuda.current_stream(device).cuda_stream)

    def apply_torch(self, table, packed, used, *, idle=0, out=None, expect=None, report=None):
        """table: (batch, max_segments, 3) int32, packed: (batch, >= width * capacity) int16, used: contiguous
        (batch, 2) int64 (rows may be windows of wider tensors); idle: one int16 code or one per code of a sample; out:
        (batch, >= width * n) int16; expect: the same, or None; report: contiguous (batch, 4) int64 -- out and report
        allocated when None.  out may share memory with no input, expect among them (ValueError); the inputs are never
        written.  Asynchronous on torch's current stream, no allocation when the outputs are given.
        -> (out[:, :width * n], report)"""
        import torch
        k, rows = self.width, self.batch
        try:
            idle = _engine.segment_play_idle(idle, k)
        except ValueError as e:
            raise ValueError(f'segment play: {e}') from None
        sides, t0, ts, p0, ps, u0, e0, es = self._inputs(table, packed, used, expect)
        if out is None:
            out = torch.empty((rows, max(k * self.n, 1)), dtype=torch.int16, device=table.device)[:, :k * self.n]
        o0, os_ = _rows.check_rows(out, rows, k * self.n, _rows.torch_dtype(np.int16),
                                   'expected out: (batch, >=width * n) row-contiguous int16 device tensor')
        side = (o0, os_, rows, k * self.n, 2)
        for name, s in sides:
            if not _rows.rows_disjoint(side, s):
                raise ValueError(f'segment play: out overlaps {name}')
        report, r0 = self._report(report, sides + [('out', side)], table.device)
        self._launch(table.device, t0, ts, p0, ps, u0, idle, o0, os_, e0, es, r0)
        return out[:, :k * self.n], report

    def verify_torch(self, table, packed, used, expect, *, idle=0, report=None):
        """the verifying pass: the comparison of what would be played with `expect`, without an `out`; only `report`
        (allocated when None) is written.  -> report"""
        if expect is None:
            raise ValueError('expected expect: (batch, >=width * n) row-contiguous int16 device tensor')
        try:
            idle = _engine.segment_play_idle(idle, self.width)
        except ValueError as e:
            raise ValueError(f'segment play: {e}') from None
        sides, t0, ts, p0, ps, u0, e0, es = self._inputs(table, packed, used, expect)
        report, r0 = self._report(report, sides, table.device)
        self._launch(table.device, t0, ts, p0, ps, u0, idle, None, 0, e0, es, r0)
        return report

    def check_torch(self, table, packed, used, report=None):
        """the checking pass: is every row good, and how much does it play; only `report` (allocated when None) is
        written, [played, 0, 0, -1] or all -1.  -> report"""
        sides, t0, ts, p0, ps, u0, _, _ = self._inputs(table, packed, used, None)
        report, r0 = self._report(report, sides, table.device)
        self._launch(table.device, t0, ts, p0, ps, u0, (0, 0), None, 0, None, 0, r0)
        return report

    def close(self):
        if self.plan is not None:
            self.plan.close()
            self.plan = None


def play_rows(segments, n, idle=0, width=1, expect=None, return_report=False):
    """The rows that `segments` play (see `SegmentPlayer`), all rows in one apply: NumPy in, NumPy out.  `segments`: a
    list of (table_r (count_r, 3) int32, packed_r int16), one per row, as `segment_rows` returns them -- or
    (plays_r, library_r) of what `library_rows` returns; `idle`: one int16 code or one per code of a sample; `expect`:
    (rows, width * n) int16 or None.  -> out (rows, width * n) int16, with `return_report` (out, report (rows, 4) int64
    [played, differ, stray, first]).  ValueError before any device work: no rows, a width other than 1 or 2, a table
    that is not (count, 3) int32, packed codes that are not 1-D int16 or no multiple of the width, an expect of
    another shape or dtype, an idle that is not one code or one per code of a sample, what `SegmentPlayer` refuses;
    ValueError after it, naming the row: a row that is not good."""
    if width not in (1, 2):
        raise ValueError('play_rows: width must be 1 or 2')
    k = int(width)
    try:
        segments = [(np.asarray(t), np.asarray(p)) for t, p in segments]
    except (TypeError, ValueError):
        raise ValueError('play_rows: segments must be a list of (table, packed) pairs') from None
    rows = len(segments)
    if rows < 1:
        raise ValueError('play_rows: no rows')
    for r, (t, p) in enumerate(segments):
        if t.ndim != 2 or t.shape[1] != 3 or t.dtype != np.int32:
            raise ValueError(f'play_rows: row {r}: the table must be (count, 3) int32')
        if p.ndim != 1 or p.dtype != np.int16 or len(p) % k:
            raise ValueError(f'play_rows: row {r}: the packed codes must be 1-D int16, a multiple of the width long')
    ms, cap = max(len(t) for t, _ in segments), max(len(p) for _, p in segments) // k
    try:
        n, rows, k, ms, cap = _engine.segment_play_arguments(n, rows, k, ms, cap)
        idle = _engine.segment_play_idle(idle, k)
    except ValueError as e:
        raise ValueError(f'play_rows: {e}') from None
    if expect is not None:
        expect = np.asarray(expect)
        if expect.shape != (rows, k * n) or expect.dtype != np.int16:
            raise ValueError(f'play_rows: expect must be an int16 array of the shape ({rows}, {k * n})')
        expect = np.ascontiguousarray(expect)
    table = np.zeros((rows, max(ms, 1), 3), dtype=np.int32)
    packed = np.zeros((rows, max(k * cap, 1)), dtype=np.int16)
    used = np.zeros((rows, 2), dtype=np.int64)
    for r, (t, p) in enumerate(segments):
        table[r, :len(t)] = t
        packed[r, :len(p)] = p
        used[r] = len(t), len(p) // k
    nbytes = max(rows * k * n * 2, 16)
    with _engine.SegmentPlayPlan(n, rows, k, ms, cap) as plan, _engine.DeviceBuffer(table.nbytes) as t, \
            _engine.DeviceBuffer(packed.nbytes) as y, _engine.DeviceBuffer(used.nbytes) as u, \
            _engine.DeviceBuffer(nbytes) as o, _engine.DeviceBuffer(nbytes) as e, \
            _engine.DeviceBuffer(rows * 32) as rp:
        t.upload(table)
        y.upload(packed)
        u.upload(used)
        if expect is not None and n:
            e.upload(expect)
        plan.apply(t.ptr if ms else None, table.shape[1] * 3, y.ptr if cap else None, packed.shape[1], u.ptr, idle,
                   o.ptr if n else None, k * n, e.ptr if expect is not None and n else None, k * n, rp.ptr)
        _engine.sync()
        report = rp.download((rows, 4), np.int64)
        out = o.download((rows, k * n), np.int16) if n else np.zeros((rows, 0), dtype=np.int16)
    for r in range(rows):
        if report[r, 0] < 0:
            raise ValueError(f'play_rows: row {r}: the table cannot be played: its entries must be non-empty, '
                             f'ascending, disjoint, inside the row of {n} samples and inside the packed codes')
    return (out, report) if return_report else out


def _extract_taps(name, n, sample_rate, bw):
    """the smoothing taps of extractKernel for rows of n samples, by the reference's own expressions
    (distortion.py:45-47), or None where it does not smooth (bw is None or bw >= sample_rate / 2).  ValueError: a
    sample_rate or bw that is not finite, bw <= 0, more taps than samples."""
    sample_rate = float(sample_rate)
    if not np.isfinite(sample_rate):
        raise ValueError(f'{name}: sample_rate is not finite')
    if bw is None:
        return None
    bw = float(bw)
    if not np.isfinite(bw) or bw <= 0.0:
        raise ValueError(f'{name}: bw must be finite and positive (or None)')
    if not bw < 0.5 * sample_rate:
        return None
    m = int(2 * sample_rate / bw)
    if m > n:
        raise ValueError(f'{name}: bw gives {m} smoothing taps for rows of {n} samples; the reference returns '
                         f'{m} samples there, rows keep their length here, so it is refused')
    g = np.exp(-0.5 * np.linspace(-3.0, 3.0, m)**2)
    return g / g.sum()


def _extract_skip(name, skip):
    skip = int(skip)
    if skip < 0:
        raise ValueError(f'{name}: skip must not be negative')
    return skip


class KernelExtractor:
    """Device-resident `extractKernel` for `batch` rows of `n` float64 samples (build once, apply whenever the lines
    are measured again): row r of the result is the reference's
        extractKernel(sig_in[r], sig_out[r], sample_rate, bw, skip)                      (distortion.py:42-48)
    -- the centred inverse transform of fft(sig_in) / fft(sig_out), smoothed with the reference's +-3 sigma Gaussian
    of int(2 * sample_rate / bw) points when `bw < sample_rate / 2`, `skip` samples cut at each end -- i.e. the rows
    of the kernel matrix `FirStage(ker, ...)` takes.  `shared_input`: one `sig_in` (the programmed waveform) for all
    rows; it is transformed once per apply.  `.k` = max(n - 2 skip, 0) samples per result row, `.taps` the smoothing
    taps (None: no smoothing; bit for bit the reference's), `.n`, `.batch`.
    Two departures from the reference, on purpose: a `bw` that gives more taps than a row has samples is refused
    (np.convolve 'same' returns that many samples there; rows keep their length here), and so is a negative `skip`
    (ValueError both, before any device work).  A zero bin in the transform of a `sig_out` row makes that row's
    result non-finite, as in the reference; other rows are not affected.

        ex = KernelExtractor(n, lines, 2e9, bw=0.2e9, skip=(n - 1025) // 2, shared_input=True)
        ker = ex.apply_torch(programmed, measured)          # (lines, ex.k), on torch's current stream
        fir = FirStage(ker.cpu().numpy(), n, lines)
    """

    def __init__(self, n: int, batch: int, sample_rate: float, bw=None, skip: int = 0, shared_input: bool = False):
        n, batch = int(n), int(batch)
        if n < 1 or batch < 1:
            raise ValueError('KernelExtractor: n >= 1 and batch >= 1')
        skip = _extract_skip('KernelExtractor', skip)
        taps = _extract_taps('KernelExtractor', n, sample_rate, bw)
        self.plan = _engine.ExtractRowsPlan(n, batch, taps, skip, shared_input)
        self.n, self.batch, self.skip, self.k = self.plan.n, self.plan.batch, self.plan.skip, self.plan.k
        self.taps, self.shared_input = self.plan.taps, self.plan.shared_input
        self.sample_rate, self.bw = float(sample_rate), bw

    def apply(self, sig_in_ptr, in_stride, sig_out_ptr, out_sig_stride, ker_ptr, ker_stride, stream=0):
        self.plan.apply(sig_in_ptr, in_stride, sig_out_ptr, out_sig_stride, ker_ptr, ker_stride, stream)

    def kernel_name(self) -> str:
        return self.plan.kernel_name()

    def apply_torch(self, sig_in, sig_out, out=None):
        """sig_in, sig_out: (batch, >= n) row-contiguous float64 device tensors (rows may be windows of a wider
        tensor; they may overlap each other); a shared `sig_in` is 1-D of >= n samples or (1, >= n).  out: None
        (allocated) or a (batch, >= k) tensor of the same kind whose rows share no memory with an input (ValueError).
        Asynchronous on torch's current stream; one extractor serves one stream at a time (it owns the transform
        buffers).  -> out[:, :k]"""
        import torch
        f64 = _rows.torch_dtype(np.float64)
        in_rows = 1 if self.shared_input else self.batch
        if self.shared_input and sig_in.dim() == 1:
            sig_in = sig_in[None, :]
        message = 'expected row-contiguous float64 device tensors: sig_in ({}, >=n), sig_out (batch, >=n)'.format(
            1 if self.shared_input else 'batch')
        a0, a_s = _rows.check_rows(sig_in, in_rows, self.n, f64, message)
        b0, b_s = _rows.check_rows(sig_out, self.batch, self.n, f64, message)
        if out is None:
            out = torch.empty((self.batch, self.k), dtype=f64, device=sig_out.device)
        y0, y_s = _rows.check_rows(out, self.batch, self.k, f64,
                                   'out must be a (batch, >=k) row-contiguous float64 device tensor')
        y = (y0, y_s, self.batch, self.k, 8)
        if not (_rows.rows_disjoint(y, (a0, a_s, in_rows, self.n, 8))
                and _rows.rows_disjoint(y, (b0, b_s, self.batch, self.n, 8))):
            raise ValueError('kernel extraction is out of place: out overlaps an input')
        if self.k:
            self.apply(a0, a_s, b0, b_s, y0, y_s, torch.cuda.current_stream(sig_out.device).cuda_stream)
        return out[:, :self.k]

    def close(self):
        self.plan.close()


def extract_kernel_rows(sig_in, sig_out, sample_rate, bw=None, skip=0):
    """`extractKernel(sig_in[r], sig_out[r], sample_rate, bw, skip)` for every row r of a 2-D `sig_out` (reference
    distortion.py:42-48 per row), all rows in one apply, NumPy in and out: -> (rows, max(n - 2 skip, 0)) float64.
    `sig_in`: 2-D of the same shape, or 1-D of n samples (one programmed waveform for all rows).  See
    `KernelExtractor` for the operation and its two departures from the reference: a `bw` that gives more smoothing
    taps than a row has samples is refused, and a negative `skip` is refused.  ValueError before any device work:
    sig_out not 2-D, sig_in neither 1-D nor 2-D or of another shape, skip < 0, more taps than samples, a sample_rate /
    bw that is not finite, bw <= 0.  NotImplementedError: complex rows.  No rows, no samples or nothing left after
    the crop: an empty array, without a device."""
    name = 'extract_kernel_rows'
    b = np.asarray(sig_out)
    a = np.asarray(sig_in)
    if b.ndim != 2:
        raise ValueError(f'{name}: sig_out must be 2-D (rows, samples)')
    if a.ndim not in (1, 2):
        raise ValueError(f'{name}: sig_in must be 2-D like sig_out, or 1-D (one input for all rows)')
    batch, n = b.shape
    if (a.ndim == 2 and a.shape != b.shape) or (a.ndim == 1 and a.shape[0] != n):
        raise ValueError(f'{name}: sig_in has shape {a.shape}, sig_out {b.shape}')
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        raise NotImplementedError(f'{name}: complex rows')
    skip = _extract_skip(name, skip)
    taps = _extract_taps(name, n, sample_rate, bw)
    k = max(n - 2 * skip, 0)
    if n == 0 or batch == 0 or k == 0:
        return np.empty((batch, k), dtype=np.float64)
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    with _engine.ExtractRowsPlan(n, batch, taps, skip, a.ndim == 1) as plan, _engine.DeviceBuffer(a.nbytes) as xa, \
            _engine.DeviceBuffer(b.nbytes) as xb, _engine.DeviceBuffer(batch * k * 8) as y:
        xa.upload(a)
        xb.upload(b)
        plan.apply(xa.ptr, n, xb.ptr, n, y.ptr, k)
        _engine.sync()
        return y.download((batch, k), np.float64)


def zDistortKernel(dt, params):
    """FIR kernel of a Z-line distortion model (filter DESIGN: one small FFT on the host,
    reference: distortion.py:52-60)."""
    t = 3 * np.asarray(params)[:, 0].max()
    omega = 2 * np.pi * np.fft.fftfreq(int(t / dt) + 1, dt)
    H = 1
    for tau, A in params:
        H = H + (1j * A * omega * tau) / (1j * omega * tau + 1)
    return np.fft.ifftshift(np.fft.ifft(1 / H)).real


def high_pass_filter(tau, sample_rate):
    """reference: distortion.py:63-70"""
    k = 2.0 * tau * sample_rate
    return [k / (1 + k), -k / (1 + k)], [1.0, (1 - k) / (1 + k)]


# --------------------------------------------------------------------------
# filter-design helpers (host, O(order) or one short FFT: design time, not the data path)
# --------------------------------------------------------------------------
def extractKernel(sig_in, sig_out, sample_rate, bw=None, skip=0):
    """Deconvolution kernel that maps `sig_out` back onto `sig_in` (reference:
    distortion.py:42-48): centred inverse FFT of the spectral ratio, optionally smoothed
    with a +-3 sigma Gaussian of `2*sample_rate/bw` points, `skip` samples cut at each end."""
    ratio = np.fft.fft(sig_in) / np.fft.fft(sig_out)
    ker = np.fft.ifftshift(np.fft.ifft(ratio)).real
    if bw is not None and bw < 0.5 * sample_rate:
        g = np.exp(-0.5 * np.linspace(-3.0, 3.0, int(2 * sample_rate / bw))**2)
        ker = np.convolve(ker, g / g.sum(), mode='same')
    return ker[int(skip):len(ker) - int(skip)]


def exp_decay_filter_old(amp, tau, sample_rate):
    """First-order section of H(w) = A / (1 - 1j/(w tau)) in the reference's earlier
    discretisation (distortion.py:73-99) -> (b, a)."""
    decay = np.exp(-1 / (abs(sample_rate * tau) * (1 + amp)))      # = 1 - alpha
    alpha = 1 - decay
    if amp >= 0:
        k = amp / (1 + amp - alpha)
        a0, a1 = 1 - k + k * alpha, -(1 - k) * (1 - alpha)
    else:
        k = -amp / (1 + amp) / (1 - alpha)
        a0, a1 = 1 + k - k * alpha, -(1 + k) * (1 - alpha)
    return [1 / a0, -(1 - alpha) / a0], [1, a1 / a0]


def factor_filter(b, a):
    """Split (b, a) into first-order sections, one per pole/zero pair, the gain spread
    evenly over them (reference: distortion.py:247-265).  Note np.poly1d indexing: `b[0]`
    is the CONSTANT coefficient, as in the reference."""
    from itertools import zip_longest
    bp, ap = np.poly1d(b), np.poly1d(a)
    poles, zeros = ap.roots, bp.roots
    gain = (bp[0] / ap[0])**(1 / max(len(zeros), len(poles)))
    return [([gain, -gain * z], [1, -p]) for p, z in zip_longest(poles, zeros, fillvalue=0)]


def stable_filter(exp_decay_filters, sample_rate):
    """True when every pole of the combined exp-decay cascade lies inside the unit circle
    (reference: distortion.py:268-286; it unpacks exp_decay_filter's (b, a) as (a, b) and
    swaps them back when combining, which is kept)."""
    from scipy.signal import tf2zpk
    pairs = []
    for amp, tau in exp_decay_filters:
        first, second = exp_decay_filter(amp, tau, sample_rate)
        pairs.append((second, first))
    b, a = combine_filters(pairs)
    _, poles, _ = tf2zpk(b, a)
    return bool(np.all(np.abs(poles) < 1))
