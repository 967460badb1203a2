"""Referee of the per-row kernel extraction (distortion.KernelExtractor / extract_kernel_rows): the five steps of the
reference's extractKernel(sig_in, sig_out, sample_rate, bw, skip) per row, written from their definition in NumPy and
evaluated twice, in float64 (numpy.fft) and in np.longdouble (scipy.fft transforms long doubles natively):

    1. R[k] = rfft(sig_in)[k] / rfft(sig_out)[k],  k = 0 .. n // 2
    2. c = irfft(R, n)
    3. s[i] = c[(i + n // 2) mod n]                                                    (ifftshift)
    4. t[i] = sum_m g[m] s[i + (M - 1) // 2 - m], s = 0 outside [0, n)                 (np.convolve 'same', M <= n)
       with g = exp(-0.5 * linspace(-3, 3, M)**2), g /= g.sum(), M = int(2 * sample_rate / bw), when bw is given and
       bw < 0.5 * sample_rate; t = s otherwise
    5. out[j] = t[j + skip],  0 <= j < K = max(n - 2 skip, 0)

Bound of the device against the long-double result, per row: max(1e-12 * scale, 10 * self_err), scale = max |long
double result| of the row, self_err = max |float64 leg - long double leg| of the row.  1e-12 * scale is what
tests/test_symbolic_cpu.py holds extractKernel to against the reference's goldens; 10 * self_err is DESIGN 7 (iv)'s
form.  So that the second term cannot hide a failure, `rows_ref` asserts self_err <= 1e-13 * scale for every row of
every case: the floor governs everywhere, and no case is dropped for its conditioning.
"""
import numpy as np
import scipy.fft

FLOOR = 1e-12          # times scale
SELF_ERR_MAX = 1e-13   # times scale: the condition on every case


def make_input(n, seed):
    """the recipe of tests/cases.extract_input: a random walk plus noise, and its image under a short exponential
    kernel plus 0.3 of itself (a transfer function without zeros near the unit circle)"""
    rng = np.random.default_rng(seed)
    a = np.cumsum(rng.normal(size=n)) / 20 + rng.normal(size=n)
    k = np.exp(-np.arange(24) / 5.0)
    b = np.convolve(a, k / k.sum(), mode='full')[:n] + 0.3 * a
    return a, b


def taps_of(sample_rate, bw):
    """the reference's smoothing taps (its expressions, float64), or None where it does not smooth"""
    if bw is None or not bw < 0.5 * sample_rate:
        return None
    g = np.exp(-0.5 * np.linspace(-3.0, 3.0, int(2 * sample_rate / bw))**2)
    return g / g.sum()


def bw_for(M, sample_rate):
    """a bw for which int(2 * sample_rate / bw) is M (M >= 4: bw < sample_rate / 2)"""
    bw = 2 * sample_rate / (M + 0.5)
    assert int(2 * sample_rate / bw) == M and bw < 0.5 * sample_rate
    return bw


def extract_ref(a, b, g=None, skip=0, dtype=np.float64):
    """one row -> the five steps in `dtype` (float64: numpy.fft; longdouble: scipy.fft).  g: the taps or None."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    n = len(a)
    fft = np.fft if dtype == np.float64 else scipy.fft
    with np.errstate(divide='ignore', invalid='ignore'):
        R = fft.rfft(a) / fft.rfft(b)
        c = fft.irfft(R, n)
    assert c.dtype == dtype, c.dtype
    s = c[(np.arange(n) + n // 2) % n]
    if g is not None:
        M = len(g)
        assert M <= n
        with np.errstate(invalid='ignore'):
            s = np.convolve(s, np.asarray(g, dtype=dtype), mode='full')[(M - 1) // 2:(M - 1) // 2 + n]
    return s[skip:max(n - skip, skip)]


class Ref:
    """the referee's result for a batch: `want` (rows, K) long double, and per row `scale`, `self_err`, `bound`"""

    def __init__(self, want, f64):
        self.want, self.f64 = want, f64
        rows, K = want.shape
        self.scale = np.array([float(np.max(np.abs(w))) if K else 0.0 for w in want])
        self.self_err = np.array([float(np.max(np.abs(w - f))) if K else 0.0 for w, f in zip(want, f64)])
        self.bound = np.maximum(FLOOR * self.scale, 10 * self.self_err)

    def crop(self, skip, rows=None, what=''):
        """the referee's result for the same rows (the first `rows` of them) with `skip` more samples cut at each end:
        step 5 is a slice, so this IS the referee at that skip, and it is held to the same condition"""
        n = self.want.shape[1]
        sl = slice(skip, max(n - skip, skip))
        ref = Ref(self.want[:rows, sl], self.f64[:rows, sl])
        ref.assert_conditioned(what)
        return ref

    def assert_conditioned(self, what=''):
        assert np.all(self.self_err <= SELF_ERR_MAX * self.scale), (what, self.self_err, self.scale)

    def check(self, got, what=''):
        """every row of `got` within its bound of the long-double result; prints the worst ratio"""
        got = np.asarray(got)
        assert got.dtype == np.float64 and got.shape == self.want.shape, (what, got.dtype, got.shape, self.want.shape)
        if not got.size:
            return
        err = np.array([float(np.max(np.abs(g.astype(np.longdouble) - w))) for g, w in zip(got, self.want)])
        ratio = err / self.bound
        print(f'{what}: worst |diff| / bound = {float(np.max(ratio)):.3g} (err {float(np.max(err)):.3g}, '
              f'scale {float(np.max(self.scale)):.3g}, self_err / scale {float(np.max(self.self_err / self.scale)):.3g})')
        assert np.all(np.isfinite(got)), f'{what}: a result is not finite'
        assert np.all(err <= self.bound), f'{what}: rows {np.nonzero(err > self.bound)[0]}: |diff| / bound = {ratio}'


def rows_ref(a_rows, b_rows, g=None, skip=0, what=''):
    """rows -> Ref; a_rows 1-D: one sig_in shared by all rows.  Asserts the condition self_err <= 1e-13 * scale."""
    b_rows = np.asarray(b_rows, dtype=np.float64)
    a_rows = np.asarray(a_rows, dtype=np.float64)
    if a_rows.ndim == 1:
        a_rows = np.broadcast_to(a_rows, b_rows.shape)
    want = np.stack([extract_ref(a, b, g, skip, np.longdouble) for a, b in zip(a_rows, b_rows)])
    f64 = np.stack([extract_ref(a, b, g, skip, np.float64) for a, b in zip(a_rows, b_rows)])
    ref = Ref(want, f64)
    ref.assert_conditioned(what)
    return ref
