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

`BinnedDemodulator` ends the same product per time bin (csrc/wfk_bdemod.hip): (shots, bins, nf), the IQ trajectory of
every shot.

Importing this module needs no GPU; creating a `Demodulator` does.
"""
from __future__ import annotations

from itertools import repeat
from types import MappingProxyType
from typing import Optional, Sequence, cast

import numpy as np
import scipy.sparse as sp

from .distortion import shift

__all__ = ['freeze', 'getFTMatrix', 'shift', 'Demodulator', 'BinnedDemodulator', 'StateDiscriminator', 'classify_points', 'TraceAverager',
           'average_traces']


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


class BinnedDemodulator:
    """The IQ trajectory of every shot on the device (csrc/wfk_bdemod.hip): `Demodulator`'s product ended per time bin,
    out[s, w, j] = sum over the samples k of bin w of traces[s, k] * e[k, j], bin w = [start + w * bin, start + (w + 1)
    * bin), w = 0 .. bins - 1 (`bins=None`: all that fit, (N - start) // bin).  e = getFTMatrix(fList, N, ...) keeps the
    global time axis, so the phases run on from bin to bin; samples before `start` and behind the last bin are not
    read, and a NaN in a sample reaches its own bin only.  fp64 throughout, a fixed order of additions.

        bd = BinnedDemodulator([f1, f2], 4096, bin=128, dtype=np.int16)
        traj = bd.apply_torch(traces)                  # (shots, >= N) device tensor -> (shots, 32, nf) complex128
        labels = disc.apply_torch(traj[:, w])          # a bin's points as StateDiscriminator takes them

    `weight=None` means np.full(N, 2 / bin) -- not getFTMatrix's 2 / N: a steady tone of amplitude A and phase phi at
    f_j then reads about A * exp(1j * phi) in EVERY bin (up to the leakage of a bin that holds no whole number of
    periods), and with start = 0 and bins * bin = N, `out.sum(1) * bin / N` is `Demodulator`'s result.  An explicit
    weight, and the matrix of `from_matrix`, are used as given.  Building one needs no GPU (the device plan is made by
    the first apply); ValueError: bin < 1, start < 0, bins < 1, start + bins * bin > N, a dtype that is not float64,
    float32 or int16, an entry of the used rows of e that is not finite."""

    def __init__(self, fList, numOfPoints, bin, start=0, bins=None, phaseList=None, weight=None, sampleRate=1e9,
                 dtype=np.float64):
        if (weight is None or len(weight) == 0) and int(bin) >= 1:
            weight = np.full(numOfPoints, 2 / int(bin))
        self._setup(getFTMatrix(fList, numOfPoints, phaseList, weight, sampleRate), bin, start, bins, dtype)

    @classmethod
    def from_matrix(cls, e, bin, start=0, bins=None, dtype=np.float64) -> 'BinnedDemodulator':
        """A binned demodulator for any (N, nf) complex matrix (matched-filter weights, ...), used as given."""
        self = cls.__new__(cls)
        self._setup(e, bin, start, bins, dtype)
        return self

    def _setup(self, e, bin, start, bins, dtype):
        from . import _engine
        self._plan = None
        self.e, self.start, self.bin, self.bins, self.dtype = _engine.bdemod_arguments(e, bin, start, bins, dtype)
        self.n, self.nf = self.e.shape

    @property
    def plan(self):
        if self._plan is None:
            from . import _engine
            self._plan = _engine.BinnedDemodPlan(self.e, self.bin, self.start, self.bins, self.dtype)
        return self._plan

    def kernel_name(self, shots: int) -> str:
        """'bdemod_tile<T,NB> groups=G': the kernel an apply on `shots` traces runs and its workgroups along the bins."""
        return self.plan.kernel_name(int(shots))

    def apply_torch(self, traces, out=None):
        """traces: (shots, >= N) row-contiguous device tensor of the plan dtype (windows x[:, w0:w0 + N] work without a
        copy).  Writes `out` (shots, bins, nf) complex128 (allocated when None; dense within a shot, any shot stride
        >= bins * nf) on torch's current stream, asynchronously, and returns it."""
        import torch
        from . import _rows
        if traces.is_complex():
            raise ValueError('complex traces are not supported')
        x_ptr, x_stride = _rows.check_rows(
            traces, None, self.n, _rows.torch_dtype(self.dtype),
            'traces must be a (shots, >= %d) row-contiguous device tensor of %s' % (self.n, self.dtype))
        shots, row = traces.shape[0], self.bins * self.nf
        if out is None:
            out = torch.empty((shots, self.bins, self.nf), dtype=torch.complex128, device=traces.device)
        message = ('out must be a (shots, %d, %d) complex128 tensor on the traces\' device, dense within a shot'
                   % (self.bins, self.nf))
        if (out.dim() != 3 or tuple(out.shape) != (shots, self.bins, self.nf) or out.device != traces.device
                or (self.bins > 1 and out.stride(1) != self.nf) or (self.nf > 1 and out.stride(2) != 1)):
            raise ValueError(message)
        flat = out.as_strided((shots, row), (out.stride(0), 1))              # a shot's bins and tones as one row
        out_ptr, out_stride = _rows.check_rows(flat, shots, row, torch.complex128, message, exact=True)
        if shots:
            stream = torch.cuda.current_stream(traces.device).cuda_stream
            self.plan.apply(x_ptr, shots, x_stride, out_ptr, out_stride, stream)
        return out

    def __call__(self, signal):
        """NumPy in, NumPy out: a real signal of shape (..., N) -> (..., bins, nf); a 1-D signal gives (bins, nf)."""
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
        return out.cpu().numpy().reshape(lead + (self.bins, self.nf))

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None


class TraceAverager:
    """Per-step sums of digitiser traces on the device (csrc/wfk_avg.hip): the reduction over SHOTS that goes with the
    demodulator's reduction over time.  The shots of a run cycle through `steps` steps (a delay sweep, the points of a
    Rabi scan); shot s of a block that `first` shots precede belongs to step (first + s) mod steps.  An apply forms,
    per step and sample, the sum of the block's traces and -- `sumsq` -- of their squares: int64 for int16 codes
    (exact), float64 for float32 / float64 traces (fixed order of additions: two applies agree to the bit).

        av = TraceAverager(N, steps=10, dtype=np.int16)
        for k, block in enumerate(blocks):                       # blocks of any length, cut anywhere in a cycle
            av.apply_torch(block, total, total_sq, first=shots_so_far, accumulate=k > 0)
        mean, var = av.finish_torch(total, total_sq, av.counts(shots_so_far))

    Building one needs no GPU (the device plan is made by the first apply); ValueError: numOfPoints < 1, steps < 1,
    a dtype that is not float64, float32 or int16."""

    def __init__(self, numOfPoints, steps=1, dtype=np.int16, sumsq=True):
        from . import _engine
        self.n, self.steps, self.dtype = _engine.avg_arguments(numOfPoints, steps, dtype)
        self.sum_dtype = np.dtype(np.int64 if self.dtype == np.dtype(np.int16) else np.float64)
        self.sumsq = bool(sumsq)
        self._plan = None

    @property
    def plan(self):
        if self._plan is None:
            from . import _engine
            self._plan = _engine.AvgPlan(self.n, self.steps, self.dtype)
        return self._plan

    def kernel_name(self, shots: int, sumsq=None) -> str:
        """Device kernel(s) an apply on `shots` traces runs (a split launch adds the reduce)."""
        return self.plan.kernel_name(int(shots), self.sumsq if sumsq is None else bool(sumsq))

    def splits(self, shots: int, first: int = 0) -> int:
        """The workgroups that share the shots of one step for a block of `shots` (1: no workspace, no reduce)."""
        return self.plan.splits(int(shots), int(first) % self.steps)

    def counts(self, shots: int, first: int = 0) -> np.ndarray:
        """(steps,) int64: how many of `shots` consecutive shots, `first` before them, belong to each step.  Host
        arithmetic, no device; with first = 0 and the run's total it is what `finish_torch` divides by."""
        shots, first = int(shots), int(first)
        if shots < 0 or first < 0:
            raise ValueError('shots and first must not be negative')
        whole, rest = divmod(shots, self.steps)
        c = np.full(self.steps, whole, dtype=np.int64)
        c[(first % self.steps + np.arange(min(rest, self.steps))) % self.steps] += 1
        return c

    def check(self, traces, sum, sumsq=None, first=0, device=True):
        """What `apply_torch` holds its tensors to, on their metadata alone (`device=False` leaves the "is a device
        tensor" clause out) -> ((ptr, stride) of traces, of sum, of sumsq or (None, 0)).  ValueError: traces that are
        not (shots, >= N) rows of the plan dtype with a row stride >= N; sum / sumsq that are not (steps, N) rows of
        int64 (int16 traces) or float64 with a row stride >= N on the traces' device; a negative first; sum or sumsq
        overlapping the traces or each other."""
        from . import _rows
        if int(first) < 0:
            raise ValueError('first must not be negative, got %d' % first)
        if traces.is_complex():
            raise ValueError('complex traces are not supported')
        x = _rows.check_rows(
            traces, None, self.n, _rows.torch_dtype(self.dtype),
            'traces must be a (shots, >= %d) row-contiguous device tensor of %s' % (self.n, self.dtype), device=device)
        shots = traces.shape[0]
        sides = [('traces', x + (shots, self.n, self.dtype.itemsize))] if shots else []
        out = []
        for name, t in (('sum', sum), ('sumsq', sumsq)):
            if t is None:
                out.append((None, 0))
                continue
            message = '%s must be a (%d, %d) row-contiguous %s tensor on the traces\' device' % (
                name, self.steps, self.n, self.sum_dtype)
            side = _rows.check_rows(t, self.steps, self.n, _rows.torch_dtype(self.sum_dtype), message, exact=True,
                                    device=device)
            if t.device != traces.device:
                raise ValueError(message)
            for other, rows in sides:
                if not _rows.rows_disjoint(side + (self.steps, self.n, 8), rows):
                    raise ValueError('trace averager is out of place: %s overlaps %s' % (name, other))
            sides.append((name, side + (self.steps, self.n, 8)))
            out.append(side)
        return x, out[0], out[1]

    def apply_torch(self, traces, sum=None, sumsq=None, first=0, accumulate=False):
        """traces: (shots, >= N) row-contiguous device tensor of the plan dtype (windows x[:, w0:w0 + N] work without
        a copy; shots = 0 and shots < steps are fine).  sum / sumsq: (steps, N) int64 (int16 traces) or float64, any row
        stride >= N; allocated when None (sumsq only if the averager was built with sumsq=True), which needs
        accumulate=False.  accumulate=False overwrites them (a step without a shot in the block gets 0);
        accumulate=True adds the block's sums to them and leaves a step without a shot bit for bit as it was.
        Asynchronous on torch's current stream.  -> sum, or (sum, sumsq)."""
        import torch
        from . import _rows
        if accumulate and (sum is None or (sumsq is None and self.sumsq)):
            raise ValueError('accumulate=True needs the tensors to add to')
        out_dtype = _rows.torch_dtype(self.sum_dtype)
        if sum is None:
            sum = torch.empty((self.steps, self.n), dtype=out_dtype, device=traces.device)
        if sumsq is None and self.sumsq:
            sumsq = torch.empty((self.steps, self.n), dtype=out_dtype, device=traces.device)
        (x_ptr, x_stride), (s_ptr, s_stride), (q_ptr, q_stride) = self.check(traces, sum, sumsq, first)
        stream = torch.cuda.current_stream(traces.device).cuda_stream
        self.plan.apply(x_ptr, traces.shape[0], x_stride, int(first) % self.steps, s_ptr, s_stride, q_ptr, q_stride,
                        accumulate, stream)
        return sum if sumsq is None else (sum, sumsq)

    def finish_torch(self, sum, sumsq, counts):
        """(mean, var) float64 (steps, N) from the sums and the shots per step (`counts(total)`): mean = sum / count,
        var = sumsq / count - mean^2 (the population variance; None without sumsq), NaN where a step has no shot.
        Plain torch ops on steps x N elements."""
        import torch
        cnt = torch.as_tensor(np.asarray(counts, dtype=np.float64), device=sum.device).reshape(self.steps, 1)
        mean = sum.to(torch.float64) / cnt
        var = None if sumsq is None else sumsq.to(torch.float64) / cnt - mean * mean
        return mean, var

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None


def average_traces(signal, steps=1, return_var=False):
    """NumPy in, NumPy out: the mean trace per step of a real (shots, N) signal whose shots cycle through `steps`
    steps from step 0 -> (steps, N) float64 mean [, var with return_var].  int16 stays int16 on the device (exact
    sums), float32 stays float32, narrower integers are read as int16 and anything else that fits as float64.  A step
    without a shot is NaN; no shots or no samples are answered without a device."""
    import torch
    signal = np.asarray(signal)
    if np.iscomplexobj(signal):
        raise ValueError('complex traces are not supported')
    if signal.ndim != 2:
        raise ValueError('signal must have shape (shots, N), got %s' % (signal.shape,))
    if int(steps) < 1:
        raise ValueError('steps >= 1, got %d' % steps)
    steps = int(steps)
    shots, n = signal.shape
    if shots == 0 or n == 0:
        nan = np.full((steps, n), np.nan)
        return (nan, nan.copy()) if return_var else nan
    dtype = next((d for d in (np.int16, np.float32, np.float64)
                  if signal.dtype == d or (d != np.float32 and np.can_cast(signal.dtype, d, 'safe'))), None)
    if dtype is None:
        raise ValueError('a %s signal fits neither int16 nor float64' % signal.dtype)
    av = TraceAverager(n, steps, dtype, sumsq=return_var)
    try:
        dev = torch.device('cuda', torch.cuda.current_device())
        x = torch.from_numpy(np.ascontiguousarray(signal, dtype=dtype)).to(dev)
        res = av.apply_torch(x)
        total, total_sq = res if return_var else (res, None)
        mean, var = av.finish_torch(total, total_sq, av.counts(shots))
        return (mean.cpu().numpy(), var.cpu().numpy()) if return_var else mean.cpu().numpy()
    finally:
        av.close()


class StateDiscriminator:
    """IQ points to qubit states and per-step counts on the device (csrc/wfk_states.hip): the link behind the
    demodulator.  `centres` is (nf, K) complex, 2 <= K <= 8, 1 <= nf <= 1024; a tone with fewer states pads its row
    with NaN.  A point takes the state of the nearest centre of its tone -- squared distance in double, every operation
    rounded on its own, so NumPy's `dr * dr + di * di` gives the same bits; ties go to the lowest state; a NaN or
    infinite distance never wins and a point no centre wins is labelled 255.  The shots of a run cycle through `steps`
    steps: shot s of a block that `first` shots precede belongs to step (first + s) mod steps.

        sd = StateDiscriminator.from_calibration(cal_iq, n_states=2, steps=10)
        counts = torch.zeros((10, sd.nf, sd.n_states + 1), dtype=torch.int64, device='cuda')
        for k, iq in enumerate(blocks):                          # blocks of any length, cut anywhere in a cycle
            sd.apply_torch(iq, counts=counts, first=shots_so_far, accumulate=k > 0)
        p = sd.probabilities(counts, sd.counts_of(shots_so_far))  # (steps, nf, K): p[:, j, 1] is P(1) of tone j

    Building one needs no GPU (the device plan is made by the first apply); ValueError: centres that are not 2-D,
    K < 2, K > 8, nf > 1024, steps < 1, a tone whose centres are all NaN."""

    INVALID = 255

    def __init__(self, centres, steps=1):
        from . import _engine
        self.centres, self.steps = _engine.states_arguments(centres, steps)
        self.nf, self.n_states = self.centres.shape
        self.bits = _engine.states_bits(self.n_states)
        self.word_bits = self.nf * self.bits
        self.joint_bins = 2 ** self.word_bits + 1 if self.word_bits <= 16 else None
        self._plan = None

    @classmethod
    def from_calibration(cls, points, n_states, first=0, steps=1) -> 'StateDiscriminator':
        """Centres from a calibration run whose shots cycle through the `n_states` prepared states: shot s (`first`
        shots before it) was prepared in state (first + s) mod n_states, and centre[j, k] is the mean of tone j over
        the shots of state k.  points: (shots, nf) complex, a tensor on any device or an array.  Plain torch ops on a
        small problem.  `steps`: of the discriminator that is returned."""
        import torch
        n_states, first = int(n_states), int(first)
        if n_states < 2:
            raise ValueError('state discriminator: n_states must lie in [2, 8], got %d' % n_states)
        if first < 0:
            raise ValueError('first must not be negative, got %d' % first)
        pts = torch.as_tensor(points)
        if pts.dim() != 2 or not pts.is_complex():
            raise ValueError('points must be (shots, nf) complex, got shape %s of %s' % (tuple(pts.shape), pts.dtype))
        pts = pts.to(torch.complex128)
        # the shots of state k are every n_states-th one from (k - first) mod n_states; a state without a shot gives NaN
        means = [pts[(k - first) % n_states::n_states].mean(dim=0) for k in range(n_states)]
        return cls(torch.stack(means, dim=1).cpu().numpy(), steps)

    @property
    def plan(self):
        if self._plan is None:
            from . import _engine
            self._plan = _engine.StatesPlan(self.centres, self.steps)
        return self._plan

    def kernel_name(self, shots: int) -> str:
        """The device kernel an apply on `shots` points runs, its block and where each table is counted."""
        return self.plan.kernel_name(int(shots))

    def counts_of(self, shots: int, first: int = 0) -> np.ndarray:
        """(steps,) int64: how many of `shots` consecutive shots, `first` before them, belong to each step.  Host
        arithmetic, no device; with first = 0 and the run's total it is what `probabilities` divides by."""
        shots, first = int(shots), int(first)
        if shots < 0 or first < 0:
            raise ValueError('shots and first must not be negative')
        whole, rest = divmod(shots, self.steps)
        c = np.full(self.steps, whole, dtype=np.int64)
        c[(first % self.steps + np.arange(min(rest, self.steps))) % self.steps] += 1
        return c

    def check(self, points, labels=None, words=None, counts=None, joint=None, first=0, device=True):
        """What `apply_torch` holds its tensors to, on their metadata alone (`device=False` leaves the "is a device
        tensor" clause out) -> ((ptr, stride) of points, (ptr, stride) of labels or (None, 0), the pointers of words,
        counts and joint or None).  ValueError: points that are not (shots, >= nf) rows of complex128 with a row stride
        >= nf; labels that are not (shots, nf) uint8 rows with a row stride >= nf; words that are not (shots,) int64
        with unit stride, or asked for with nf * bits > 62; counts that are not a contiguous (steps, nf, K + 1) int64
        tensor; joint that is not a contiguous (steps, 2^(nf bits) + 1) int64 tensor, or asked for with nf * bits >
        16; an output on another device than the points; a negative first; no output at all; an output overlapping
        the points or another output."""
        import torch
        from . import _rows
        stage = 'state discriminator'
        if int(first) < 0:
            raise ValueError('first must not be negative, got %d' % first)
        if labels is None and words is None and counts is None and joint is None:
            raise ValueError('%s: no output' % stage)
        x = _rows.check_rows(points, None, self.nf, torch.complex128,
                             'points must be a (shots, >= %d) row-contiguous device tensor of complex128' % self.nf,
                             device=device)
        shots = points.shape[0]
        sides = [('points', x + (shots, self.nf, 16))] if shots else []

        def place(name, side, t, message, report=False):
            if t.device != points.device:
                raise ValueError(message)
            for other, rows in sides:
                if not (_rows.report_disjoint(side[0], side[2], side[1], rows) if report
                        else _rows.rows_disjoint(side, rows)):
                    raise ValueError('%s is out of place: %s overlaps %s' % (stage, name, other))
            sides.append((name, side))

        lab = (None, 0)
        if labels is not None:
            message = 'labels must be a (shots, %d) row-contiguous uint8 tensor on the points\' device' % self.nf
            lab = _rows.check_rows(labels, shots, self.nf, torch.uint8, message, exact=True, device=device)
            if shots:
                place('labels', lab + (shots, self.nf, 1), labels, message)
        w_ptr = None
        if words is not None:
            if self.word_bits > 62:
                raise ValueError('%s: words need nf * bits <= 62, got %d' % (stage, self.word_bits))
            message = 'words must be a (shots,) int64 tensor of unit stride on the points\' device'
            if ((device and not words.is_cuda) or words.dtype != torch.int64 or words.dim() != 1
                    or words.shape[0] != shots or (shots > 1 and words.stride(0) != 1)):
                raise ValueError(message)
            w_ptr = words.data_ptr()
            if shots:
                place('words', (w_ptr, shots, 1, shots, 8), words, message)
        c_ptr = j_ptr = None
        if counts is not None:
            shape = (self.steps, self.nf, self.n_states + 1)
            message = 'counts must be a contiguous %s int64 tensor on the points\' device' % (shape,)
            c_ptr = _rows.check_state(counts, shape, message, device=device, dtype=np.int64)
            place('counts', (c_ptr, shape[1] * shape[2], self.steps, shape[1] * shape[2], 8), counts, message, True)
        if joint is not None:
            if self.joint_bins is None:
                raise ValueError('%s: joint needs nf * bits <= 16, got %d' % (stage, self.word_bits))
            shape = (self.steps, self.joint_bins)
            message = 'joint must be a contiguous %s int64 tensor on the points\' device' % (shape,)
            j_ptr = _rows.check_state(joint, shape, message, device=device, dtype=np.int64)
            place('joint', (j_ptr, self.joint_bins, self.steps, self.joint_bins, 8), joint, message, True)
        return x, lab, w_ptr, c_ptr, j_ptr

    def apply_torch(self, points, labels=None, words=None, counts=None, joint=None, first=0, accumulate=False):
        """points: (shots, >= nf) row-contiguous complex128 device tensor (the demodulator's output as it is, or a
        window x[:, w0:w0 + nf] of a wider one, without a copy; shots = 0 and shots < steps are fine).  The outputs are
        the caller's: labels (shots, nf) uint8, any row stride >= nf; words (shots,) int64; counts (steps, nf, K + 1)
        and joint (steps, 2^(nf bits) + 1) int64, contiguous.  With none of the four, labels are allocated.
        accumulate=False overwrites counts and joint (a step without a shot gets 0); accumulate=True adds the block's
        counts to them, which needs the tensors to add to.  Asynchronous on torch's current stream.  -> what it wrote:
        one tensor, or a tuple in the order (labels, words, counts, joint)."""
        import torch
        if accumulate and counts is None and joint is None:
            raise ValueError('accumulate=True needs the tensors to add to')
        if labels is None and words is None and counts is None and joint is None:
            if not points.is_cuda or points.dim() != 2:
                raise ValueError('points must be a (shots, >= %d) row-contiguous device tensor of complex128' % self.nf)
            labels = torch.empty((points.shape[0], self.nf), dtype=torch.uint8, device=points.device)
        (x_ptr, x_stride), (l_ptr, l_stride), w_ptr, c_ptr, j_ptr = self.check(points, labels, words, counts, joint, first)
        stream = torch.cuda.current_stream(points.device).cuda_stream
        self.plan.apply(x_ptr, points.shape[0], x_stride, int(first), l_ptr, l_stride, w_ptr, c_ptr, j_ptr,
                        accumulate, stream)
        wrote = tuple(t for t in (labels, words, counts, joint) if t is not None)
        return wrote[0] if len(wrote) == 1 else wrote

    def probabilities(self, counts, shots_per_step):
        """(steps, nf, K) float64: counts[g, j, k] / shots_per_step[g] (`counts_of(total)`) -- the invalid column is
        left out, so a row sums to less than 1 by the invalid fraction; NaN where a step has no shot.  Plain torch ops
        on the small table."""
        import torch
        shots = torch.as_tensor(np.asarray(shots_per_step, dtype=np.float64), device=counts.device).reshape(self.steps, 1, 1)
        return counts[:, :, :self.n_states].to(torch.float64) / shots

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None


def classify_points(points, centres, steps=1, return_counts=False):
    """NumPy in, NumPy out: the state of every IQ point of a complex (..., nf) array against (nf, K) centres -> labels
    (..., nf) uint8 (255: invalid) [, counts (steps, nf, K + 1) int64 with return_counts: the shots, in C order of the
    leading axes, cycle through `steps` steps from step 0].  No shots are answered without a device."""
    import torch
    sd = StateDiscriminator(centres, steps)
    points = np.asarray(points)
    if points.ndim < 1 or points.shape[-1] != sd.nf:
        raise ValueError('points must have shape (..., %d), got %s' % (sd.nf, points.shape))
    lead = points.shape[:-1]
    x = np.ascontiguousarray(points.reshape(-1, sd.nf), dtype=np.complex128)
    if x.shape[0] == 0:
        labels = np.zeros(lead + (sd.nf,), dtype=np.uint8)
        return (labels, np.zeros((sd.steps, sd.nf, sd.n_states + 1), dtype=np.int64)) if return_counts else labels
    try:
        dev = torch.device('cuda', torch.cuda.current_device())
        xt = torch.from_numpy(x).to(dev)
        labels = torch.empty((x.shape[0], sd.nf), dtype=torch.uint8, device=dev)
        counts = torch.empty((sd.steps, sd.nf, sd.n_states + 1), dtype=torch.int64, device=dev) if return_counts else None
        sd.apply_torch(xt, labels, counts=counts)
        labels = labels.cpu().numpy().reshape(lead + (sd.nf,))
        return (labels, counts.cpu().numpy()) if return_counts else labels
    finally:
        sd.close()
