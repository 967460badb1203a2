"""Drop-in for the reference's `waveforms.utils` (utils.py): `freeze`, `getFTMatrix`, `shift`, plus a
device readout demodulator.

`getFTMatrix` builds the (N, nf) complex128 matrix on the host with the reference's own float
expressions, so it is bit-identical to it.  `traces @ getFTMatrix(...)` -- demodulating `shots`
digitizer records of N points at nf multiplexed tones -- is the hot path: `Demodulator` uploads the
matrix once and runs the product as a HIP kernel (csrc/wfk_demod.hip) on float64, float32 or raw
int16 traces, in fp64.

    dm = Demodulator([f1, f2], N, sampleRate=1e9, dtype=np.int16)
    iq = dm.apply_torch(traces)          # (shots, >= N) device tensor -> (shots, nf) complex128
    iq = dm(signal)                      # NumPy in, NumPy out: signal @ e

Importing this module needs no GPU; creating a `Demodulator` does.
"""
from __future__ import annotations

from itertools import repeat
from types import MappingProxyType
from typing import Optional, Sequence, cast

import numpy as np
import scipy.sparse as sp

from .distortion import shift

__all__ = ['freeze', 'getFTMatrix', 'shift', 'Demodulator']


def freeze(x):
    """Freeze a mutable object (reference utils.py:9-32): lists / tuples -> tuples, dict ->
    MappingProxyType, set -> frozenset, bytearray -> bytes; NumPy arrays and scipy sparse matrices are
    made read-only in place."""
    if isinstance(x, (int, float, complex, str, bytes, type(None))):
        pass
    elif isinstance(x, (list, tuple)):
        return tuple([freeze(y) for y in x])
    elif isinstance(x, dict):
        return MappingProxyType({k: freeze(v) for k, v in x.items()})
    elif isinstance(x, set):
        return frozenset([freeze(y) for y in x])
    elif isinstance(x, (np.ndarray, np.matrix)):
        x.flags.writeable = False
    elif isinstance(x, sp.spmatrix):
        cast(np.ndarray, getattr(x, 'data')).flags.writeable = False
        if getattr(x, 'format') in {'csr', 'csc', 'bsr'}:
            cast(np.ndarray, getattr(x, 'indices')).flags.writeable = False
            cast(np.ndarray, getattr(x, 'indptr')).flags.writeable = False
        elif getattr(x, 'format') == 'coo':
            cast(np.ndarray, getattr(x, 'row')).flags.writeable = False
            cast(np.ndarray, getattr(x, 'col')).flags.writeable = False
    elif isinstance(x, bytearray):
        x = bytes(x)
    return x


def getFTMatrix(fList: Sequence[float],
                numOfPoints: int,
                phaseList: Optional[Sequence[float]] = None,
                weight: Optional[np.ndarray] = None,
                sampleRate: float = 1e9) -> np.ndarray:
    """(numOfPoints, nf) complex128 matrix e with e[k, j] = weight_j[k] * exp(-1j * (2 pi f_j t_k + phase_j)),
    t = np.linspace(0, N / sampleRate, N, endpoint=False): `signal @ e` demodulates `signal` at every f_j
    (reference utils.py:35-84, element for element).  `weight` defaults to 2 / N; a 1-D weight serves every
    tone, a 2-D one gives one row per tone; nf = min(len(fList), len(phaseList), rows of weight)."""
    e = []
    t = np.linspace(0, numOfPoints / sampleRate, numOfPoints, endpoint=False)
    if weight is None or len(weight) == 0:
        weight = np.full(numOfPoints, 2 / numOfPoints)
    if phaseList is None or len(phaseList) == 0:
        phase_list = np.zeros_like(fList)
    else:
        phase_list = phaseList
    if weight.ndim == 1:
        weight_list = repeat(weight)
    else:
        weight_list = weight
    for f, phase, weight in zip(fList, phase_list, weight_list):
        e.append(weight * np.exp(-1j * (2 * np.pi * f * t + phase)))
    return np.asarray(e).T


_DTYPES = (np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.int16))


class Demodulator:
    """`traces @ e` on the device for real traces of one dtype (float64, float32 or int16 ADC codes) and a
    fixed complex (N, nf) matrix e, in fp64 (NumPy's complex128 product, up to summation order).
    Build once (the matrix is uploaded once), apply many times."""

    def __init__(self, fList, numOfPoints, phaseList=None, weight=None, sampleRate=1e9, dtype=np.float64):
        self._setup(getFTMatrix(fList, numOfPoints, phaseList, weight, sampleRate), dtype)

    @classmethod
    def from_matrix(cls, e, dtype=np.float64) -> 'Demodulator':
        """A demodulator for any (N, nf) complex matrix (matched-filter weights, ...)."""
        self = cls.__new__(cls)
        self._setup(e, dtype)
        return self

    def _setup(self, e, dtype):
        e = np.asarray(e)
        if e.ndim != 2 or e.shape[0] < 1 or e.shape[1] < 1:
            raise ValueError('the matrix must be (N, nf) with N >= 1 and nf >= 1, got shape %s' % (e.shape,))
        dtype = np.dtype(dtype)
        if dtype not in _DTYPES:
            raise ValueError('trace dtype must be float64, float32 or int16, got %s' % dtype)
        self.e = np.ascontiguousarray(e, dtype=np.complex128)
        self.n, self.nf = self.e.shape
        self.dtype = dtype
        self.plan = None
        from . import _engine
        self.plan = _engine.DemodPlan(self.e, dtype)

    def kernel_name(self, shots: int) -> str:
        """Device kernel(s) an apply on `shots` traces runs (split launches add the reduce)."""
        return self.plan.kernel_name(int(shots))

    def apply_torch(self, traces, out=None):
        """traces: (shots, >= N) row-contiguous device tensor of the plan dtype (windows x[:, w0:w0 + N] work
        without a copy).  Writes `out` (shots, nf) complex128 (allocated when None; any row stride) on
        torch's current stream, asynchronously, and returns it."""
        import torch
        from . import _rows
        if traces.is_complex():
            raise ValueError('complex traces are not supported')
        x_ptr, x_stride = _rows.check_rows(
            traces, None, self.n, _rows.torch_dtype(self.dtype),
            'traces must be a (shots, >= %d) row-contiguous device tensor of %s' % (self.n, self.dtype))
        shots = traces.shape[0]
        if out is None:
            out = torch.empty((shots, self.nf), dtype=torch.complex128, device=traces.device)
        message = 'out must be a (shots, %d) row-contiguous complex128 tensor on the traces\' device' % self.nf
        out_ptr, out_stride = _rows.check_rows(out, shots, self.nf, torch.complex128, message, exact=True)
        if out.device != traces.device:
            raise ValueError(message)
        if shots:
            stream = torch.cuda.current_stream(traces.device).cuda_stream
            self.plan.apply(x_ptr, shots, x_stride, out_ptr, out_stride, stream)
        return out

    def __call__(self, signal):
        """NumPy in, NumPy out: `signal @ e` for a real signal of shape (..., N); a 1-D signal gives (nf,)."""
        import torch
        signal = np.asarray(signal)
        if np.iscomplexobj(signal):
            raise ValueError('complex traces are not supported')
        if signal.ndim < 1 or signal.shape[-1] != self.n:
            raise ValueError('signal must have shape (..., %d), got %s' % (self.n, signal.shape))
        if not np.can_cast(signal.dtype, self.dtype, 'safe'):
            raise ValueError('a %s signal does not fit a %s demodulator' % (signal.dtype, self.dtype))
        lead = signal.shape[:-1]
        x = np.ascontiguousarray(signal.reshape(-1, self.n), dtype=self.dtype)
        dev = torch.device('cuda', torch.cuda.current_device())
        xt = torch.from_numpy(x).to(dev)
        out = self.apply_torch(xt)
        return out.cpu().numpy().reshape(lead + (self.nf,))

    def close(self):
        if self.plan is not None:
            self.plan.close()
