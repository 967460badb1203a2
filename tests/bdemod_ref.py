"""The referee of the binned demodulator (utils.BinnedDemodulator, csrc/wfk_bdemod.hip), in NumPy on the host.

Real traces x (S, >= N) of float64, float32 or int16 codes, a complex (N, nf) matrix e, three integers start >= 0,
bin >= 1 and bins = W >= 1 with start + W * bin <= N (`bins=None`: all that fit, (N - start) // bin):

    bin w covers the samples [start + w * bin, start + (w + 1) * bin)
    out[s, w, j] = SUM over k in bin w of x[s, k] * e[k, j]           (S, W, nf) complex128

in float64 after widening, e on the global time axis.  Samples before `start` and behind the last bin take no part: a
sample outside a bin is left out of the sum, not multiplied by zero.  The device's sums are held to
|device - binned| <= 1e-12 * bound, bound[s, w, j] = SUM over the bin of |x[s, k]| |e[k, j]| (test_gpu_demod.py's
bound, per bin).  A plain module like avg_ref.py."""
import numpy as np


def bins_of(n, bin, start=0, bins=None):
    """W: `bins`, or all the bins that fit"""
    return (int(n) - int(start)) // int(bin) if bins is None else int(bins)


def bin_of(k, bin, start, bins):
    """the bin sample k belongs to, None for a sample in front of `start` or behind the last bin"""
    w = (int(k) - int(start)) // int(bin)
    return w if k >= start and w < bins else None


def _used(x, e, bin, start, bins):
    """the samples and the rows of e that the bins cover, cut into bins: (W, S, bin) float64 and (W, bin, nf) complex128"""
    x, e = np.asarray(x), np.asarray(e, dtype=np.complex128)
    W = bins_of(e.shape[0], bin, start, bins)
    assert x.ndim == 2 and start >= 0 and bin >= 1 and W >= 1 and start + W * bin <= e.shape[0] <= x.shape[1]
    xs = x[:, start:start + W * bin].astype(np.float64).reshape(x.shape[0], W, bin).transpose(1, 0, 2)
    return xs, e[start:start + W * bin].reshape(W, bin, e.shape[1])


def binned(x, e, bin, start=0, bins=None):
    """(S, W, nf) complex128: one real product per bin for the real and one for the imaginary part"""
    xs, es = _used(x, e, bin, start, bins)
    out = np.matmul(xs, es.real) + 1j * np.matmul(xs, es.imag)
    return np.ascontiguousarray(out.transpose(1, 0, 2))


def magnitude(x, e, bin, start=0, bins=None):
    """(S, W, nf) float64: SUM over the bin of |x| |e|, what the parity bound is 1e-12 of"""
    xs, es = _used(x, e, bin, start, bins)
    return np.ascontiguousarray(np.matmul(np.abs(xs), np.abs(es)).transpose(1, 0, 2))


def brute_force(x, e, bin, start=0, bins=None):
    """the same by a Python loop over shots, bins, tones and samples, in Python floats"""
    x, e = np.asarray(x), np.asarray(e, dtype=np.complex128)
    W = bins_of(e.shape[0], bin, start, bins)
    out = np.zeros((x.shape[0], W, e.shape[1]), dtype=np.complex128)
    for s in range(x.shape[0]):
        for w in range(W):
            for j in range(e.shape[1]):
                re = im = 0.0
                for k in range(start + w * bin, start + (w + 1) * bin):
                    v = float(x[s, k])
                    re += v * float(e[k, j].real)
                    im += v * float(e[k, j].imag)
                out[s, w, j] = complex(re, im)
    return out


def bin_groups(shots, nf, bins):
    """the bin-group rule (include/wfk.h, wfk_bdemod_bin_groups): workgroups along the bin axis"""
    if shots < 1 or nf < 1 or bins < 1:
        return 0
    nb = 4 if nf <= 4 else 8 if nf <= 8 else 16 if nf <= 16 else 32
    blocks = -(-shots // 64) * -(-nf // nb)
    groups = min(max(1, 1024 // blocks), max(1, bins // 4))
    per_group = -(-bins // groups)
    return -(-bins // per_group)
