"""Float rows held to the double result ROUNDED ONCE, element by element ("Float forms"): the bound, the
shared input, the cascades, the float64 referees and the deliberately wrong host forms, for tests/test_float_rows_cpu.py
(which gives the bound its teeth without a device) and tests/test_gpu_float_rows.py (which holds the kernels to it).
NumPy and SciPy only; nothing here touches a device.

The bound.  A class-A kernel widens each float sample (exact), computes in double and narrows ONCE at the store.  Let w be
the referee's float64 value of an element, d the device's float64 value before the store, S = max(1, max|w|) and tol64 the
bound the form's own test file already holds double rows to, |d - w| <= tol64 * S (S per row).  The stored float is fl(d), and

    |fl(d) - w| <= |fl(d) - d| + |d - w| <= 2^-24 |d| + tol64 S <= 2^-24 |w| + (1 + 2^-24) tol64 S.

round_once_bound allows 2^-24 |w| + 2 tol64 S: the second tol64 covers a d that sits tol64 S from w on the far side of a
rounding boundary, i.e. it lets the referee's own rounding (fl(w), the number a reader would compute) stand in for w
without a second argument.  Neither number is tuned to what a device gives.

Exactly rounded.  If fl(d) != fl(w) a float32 rounding boundary (the midpoint of two neighbouring floats) lies between d
and w, so w is within tol64 S of that boundary.  Wherever w is further than 2 tol64 S from both boundaries of its float,
a round-once kernel returns fl(w) bit for bit: check_exactly_rounded.
"""
import numpy as np
from scipy.signal import butter, fftconvolve, lfilter

from waveforms_amd.distortion import combine_filters, exp_decay_filter

EPS32 = 2.0**-24
# the bounds the forms' own test files hold DOUBLE rows to, as fractions of max(1, peak) (tests/cases.py where they have a
# name): repeated here so that this module imports nothing that imports a device
TOL64_SINGLE_PASS = 1e-11      # tests/test_gpu_iir.py, tests/test_gpu_row_windows.py IIR_CASES: one pass, state dimension <= 4
TOL64_GAIN = 1e-15             # a bare gain (IIR_CASES['gain'])
TOL64_ROWS = 1e-9              # tests/test_gpu_iir_rows.py: per-row cascades against scipy
INITIAL = 0.25                 # the shared cascades' level (tests/test_gpu_row_windows.py)
TILE = 4096                    # samples iir_rows_tile takes per step
N_ROWS = 2 * TILE + 1717       # per-row cascades: two whole tiles and a ragged third
N_AWG = 20000                  # the sampler -> IIR chain: 10 us at 2 GS/s


# ---- the bound ------------------------------------------------------------------------------------------------------
def scale(want64):
    return max(1.0, float(np.abs(want64).max()))


def row_scale(want64):
    """S of the bound: max(1, peak) of a row -- of EACH row of a 2-D array (rows are independent in every kernel here, and
    they differ in size by 100: one S for all of them would hand the small rows the large rows' slack), shaped to broadcast"""
    a = np.abs(np.asarray(want64))
    return np.maximum(1.0, a.max(axis=-1, keepdims=True)) if a.ndim == 2 else scale(a)


def round_once_bound(want64, tol64, S=None):
    """per element: 2^-24 |want64| + 2 tol64 S, S = max(1, max |want64|) of the element's row (derivation: the module's
    docstring).  A caller that checks one COMPONENT of complex rows passes the S of the complex result."""
    want64 = np.asarray(want64, dtype=np.float64)
    return EPS32 * np.abs(want64) + 2.0 * tol64 * (row_scale(want64) if S is None else S)


def report(got32, want64, bound):
    """-> (worst |diff| / bound, its index, share of samples over the bound, worst |diff| / peak)"""
    want64 = np.asarray(want64, dtype=np.float64)
    diff = np.abs(np.asarray(got32, dtype=np.float64) - want64)
    ratio = diff / bound
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at), float(np.mean(diff > bound)), float(diff.max()) / scale(want64)


def check(got32, want64, tol64, what, extra=None, S=None):
    """|got32 - want64| <= round_once_bound(want64, tol64) (+ extra, per element) on every element; prints the worst
    ratio and on failure says where, how many and how far in fractions of the peak"""
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == np.shape(want64), (what, got32.dtype, got32.shape)
    assert np.all(np.isfinite(got32)), f'{what}: not finite'
    bound = round_once_bound(want64, tol64, S)
    if extra is not None:
        bound = bound + extra
    worst, at, share, of_peak = report(got32, want64, bound)
    text = (f'{what}: worst |diff| / bound = {worst:.3g} at {at}, {100 * share:.3g} % of the samples over the bound, '
            f'worst |diff| / peak = {of_peak:.3g}')
    print(text)
    assert worst <= 1.0, text


def check_exactly_rounded(got32, want64, tol64, what, S=None):
    """got32 == float32(want64) bit for bit wherever want64 is further than 2 tol64 S from both rounding boundaries of
    its float (the module's docstring); prints the share of elements that were decided this way.  A caller that passes a
    PART of its rows passes the S of the whole rows."""
    want64 = np.asarray(want64, dtype=np.float64)
    f = want64.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f64 = f.astype(np.float64)
    room = np.minimum(np.abs((f64 + up) / 2 - want64), np.abs((f64 + dn) / 2 - want64))
    decided = room > 2.0 * tol64 * (row_scale(want64) if S is None else S)
    bad = decided & (np.asarray(got32) != f)
    print(f'{what}: {100 * float(np.mean(decided)):.3g} % of the elements decided, {int(bad.sum())} not the rounded referee')
    assert not bad.any(), f'{what}: {int(bad.sum())} elements are not float32(referee), first at {tuple(np.argwhere(bad)[0])}'


# ---- the shared input -------------------------------------------------------------------------------------------------
def shared_input(rows, n, seed=20260):
    """(rows, n) float32: a step x[100:6000] = 1 plus 1e-3 * normal, row r scaled by 10^(r % 3) -- a step, a long tail at
    1e-3 of it and a noise floor that keeps every sample a normal float.  float32-VALUED: widening is exact."""
    rng = np.random.default_rng(seed)
    x = 1e-3 * rng.normal(size=(rows, n))
    x[:, 100:6000] += 1.0
    x *= (10.0 ** (np.arange(rows) % 3))[:, None]
    x32 = x.astype(np.float32)
    assert np.all(np.abs(x32) >= np.finfo(np.float32).tiny)
    x32.setflags(write=False)
    return x32


def state_input(rows, D, seed=5):
    """a non-zero zi, (rows, D) float64: 0.002 * normal times the row's own size, so that the transient it starts (a
    Butterworth cascade answers a unit of state with up to 400) stays below the row's step and S stays the step's peak"""
    return np.random.default_rng(seed).normal(size=(rows, D)) * 0.002 * (10.0 ** (np.arange(rows) % 3))[:, None]


# ---- cascades ---------------------------------------------------------------------------------------------------------
def _sos(order, fc):
    return [(r[:3], r[3:]) for r in butter(order, fc, output='sos')]


def orders_of(secs):
    return [max(len(b), len(a)) - 1 for b, a in secs]


_ONEPASS_OFF = {'WFK_IIR_ONEPASS': '0'}
# The shared cascades (distortion.IirStage with one cascade for all rows):
# name -> (sections, rows, n, environment, what every pass of kernel_name() starts with, what it ends with, tol64).
# The first four are IIR_CASES of tests/test_gpu_row_windows.py with their bounds; the single sections of order 3 and 6
# are those of tests/test_gpu_iir.py (TAIL_SHAPES['order3'] at FP64_IIR_ORDER34_TOL = 5e-10; butter(6, 0.17) of
# test_iir_batch_shapes_and_properties at its 1e-10) and run the shaped lfilter builds iir_pass<float,1,3> / <float,1,6>.
SHARED_CASES = {
    'three_launch': (_sos(4, 0.07), 4, 20011, _ONEPASS_OFF, 'iir_pass<float,2,2>', '>', TOL64_SINGLE_PASS),
    'single_pass': (_sos(4, 0.07), 4, 20011, {}, 'iir_onepass<float,2,2,', '>', TOL64_SINGLE_PASS),
    'persistent': (_sos(2, 0.07), 64, 75781, {}, 'iir_onepass<float,1,2,', ' persistent', TOL64_SINGLE_PASS),
    'gain': ([([0.5], [2.0])], 5, 20011, {}, 'iir_scale<float>', '>', TOL64_GAIN),
    'order3': ([tuple(butter(3, 0.05))], 3, 20011, _ONEPASS_OFF, 'iir_pass<float,1,3>', '>', 5e-10),
    'order3_single_pass': ([tuple(butter(3, 0.05))], 3, 20011, {}, 'iir_onepass<float,1,3,', '>', 5e-10),
    'order6': ([tuple(butter(6, 0.17))], 3, 20011, {}, 'iir_pass<float,1,6>', '>', 1e-10),
}

# Per-row cascades (iir_rows_tile<float, NSEC, ORD>): the eight shapes, three rows each with constants of their own.
ROW_SHAPES = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (3, 1), (4, 1), (2, 2)]      # (n_sections, order)
ROW_RATE = 1e9
ROW_INITIAL = np.array([0.25, -0.4, 0.1])
# (amp, tau) of exp_decay_filter, a list per row; a section of order m combines m of them into ONE (b, a), as distort()
# does.  The time constants of one section are a factor >= 4 apart: direct forms of order 3 / 4 with CLUSTERED poles
# are ill-conditioned in any evaluation order (tests/test_gpu_iir_rows.py, below its GEN list), and scipy would then be
# no referee at TOL64_ROWS.  test_float_rows_cpu.py checks the referee against the long-double recurrence.
_ROW_TC = [
    [(-0.03, 2e-6), (0.015, 400e-9), (-0.01, 90e-9), (0.02, 20e-9)],
    [(0.03, 4e-6), (0.01, 700e-9), (0.02, 150e-9), (-0.03, 30e-9)],
    [(0.02, 1.5e-6), (-0.02, 300e-9), (0.01, 60e-9), (0.025, 12e-9)],
]
# ONE section of order 3 / 4: with time constants of 20 samples and more its poles sit within 0.05 of z = 1 and scipy's
# double lfilter is 1e-10 .. 1e-7 off the long-double recurrence (the same note; measured on the lists above: 7e-10 at
# order 3, 9e-8 at order 4); these spread the poles over 0.4 .. 0.99 (measured: <= 5e-12)
_ROW_TC_SPREAD = [
    [(0.02, 1.5e-9), (-0.01, 6e-9), (0.015, 25e-9), (-0.02, 120e-9)],
    [(-0.03, 2e-9), (0.02, 7e-9), (0.01, 30e-9), (0.02, 100e-9)],
    [(0.025, 1e-9), (0.01, 5e-9), (-0.02, 20e-9), (0.03, 90e-9)],
]


def row_cascades(nsec, order):
    """[[(b, a)] * nsec] * 3 rows for one shape: section s of a row combines time constants s * order .. (s + 1) * order"""
    rows = []
    for tcs in (_ROW_TC_SPREAD if order >= 3 else _ROW_TC):
        secs = []
        for s in range(nsec):
            part = tcs[s * order:(s + 1) * order]
            secs.append(combine_filters([exp_decay_filter(A, tau, ROW_RATE) for A, tau in part]))
        rows.append(secs)
    return rows


# the chain's cascades: two first-order sections per row, every row its own (2 GS/s)
CHAIN_RATE = 2e9
CHAIN_TC = [[(0.02, 20e-9), (-0.01, 900e-9)], [(-0.03, 50e-9), (0.02, 2e-6)], [(0.015, 100e-9), (0.01, 400e-9)]]
CHAIN_INITIAL = np.array([0.1, -0.2, 0.0])


def chain_cascades():
    return [[exp_decay_filter(A, tau, CHAIN_RATE) for A, tau in tcs] for tcs in CHAIN_TC]


# ---- float64 referees -------------------------------------------------------------------------------------------------
def iir_reference(secs, x, zi=None, initial=0.0, dtype=np.float64, round_sections=False):
    """scipy.signal.lfilter section by section on x - initial from zi, + initial (tests/test_gpu_row_windows.py:
    _iir_reference) -> (y, zf).  x: (rows, n); zi: (rows, D) or None.  `dtype`: the arithmetic (lfilter computes in the
    type of its arguments); `round_sections`: narrow to float32 after every section (a wrong form)."""
    x = np.asarray(x)
    y = x.astype(dtype) - dtype(initial)
    D = sum(orders_of(secs))
    zi = np.zeros((len(x), D)) if zi is None else np.asarray(zi)
    zf, off = [], 0
    for b, a in secs:
        b, a = np.asarray(b, dtype=dtype), np.asarray(a, dtype=dtype)
        m = max(len(b), len(a)) - 1
        if m == 0:
            y = y * (b[0] / a[0])
        else:
            y, z = lfilter(b, a, y, axis=-1, zi=zi[:, off:off + m].astype(dtype))
            zf.append(z)
            off += m
        if round_sections:
            y = y.astype(np.float32).astype(dtype)
    y = y + dtype(initial)
    return y, (np.concatenate(zf, axis=1) if zf else np.zeros((len(x), 0)))


def lfilter_longdouble(b, a, x, zi):
    """the lfilter recurrence (direct form II transposed) in np.longdouble, all rows at once: x (rows, n), zi (rows, m)"""
    ld = np.longdouble
    m = max(len(a), len(b)) - 1
    bb, aa = np.zeros(m + 1, dtype=ld), np.zeros(m + 1, dtype=ld)
    bb[:len(b)] = np.asarray(b, dtype=ld) / ld(a[0])
    aa[:len(a)] = np.asarray(a, dtype=ld) / ld(a[0])
    z = [np.asarray(zi[:, j], dtype=ld).copy() for j in range(m)]
    xt = np.asarray(x, dtype=ld).T.copy()
    y = np.empty_like(xt)
    for t in range(len(xt)):
        xx = xt[t]
        yy = bb[0] * xx + z[0]
        for j in range(m - 1):
            z[j] = bb[j + 1] * xx - aa[j + 1] * yy + z[j + 1]
        z[m - 1] = bb[m] * xx - aa[m] * yy
        y[t] = yy
    return y.T


def referee_self_error(secs, x, zi=None, initial=0.0):
    """max |scipy in double - the long-double recurrence| of a cascade, section by section, as a fraction of the scale"""
    x = np.asarray(x, dtype=np.float64)
    want, _ = iir_reference(secs, x, zi, initial)
    D = sum(orders_of(secs))
    zi = np.zeros((len(x), D)) if zi is None else zi
    y, off = np.asarray(x, dtype=np.longdouble) - np.longdouble(initial), 0
    for b, a in secs:
        m = max(len(b), len(a)) - 1
        y = lfilter_longdouble(b, a, y, zi[:, off:off + m]) if m else y * (np.longdouble(b[0]) / np.longdouble(a[0]))
        off += m
    y = y + np.longdouble(initial)
    return float(np.max(np.abs(want - y))) / scale(want)


def impulse_response(secs, n):
    """h[0:n] of a cascade: lfilter on a unit impulse, section by section"""
    h = np.zeros(n)
    h[0] = 1.0
    for b, a in secs:
        h = lfilter(b, a, h)
    return h


def chain_input_allowance(secs, s64, tol64_grid):
    """What the sampler part of a sampler -> IIR chain may add to one row of the float result, per element.  The kernel
    filters float32(s_dev), s_dev the device's double samples: the float row is float32(F64(float32(s_dev))).  Against
    the referee F64(s64) the INPUT is off by at most e = 2^-24 |s64| + tol64_grid * max(1, peak(s64)) (one rounding of
    the sample into the tile, plus the sampler's own fp64 bound), and a linear filter carries an input error e to at most
    |h| (*) e at its output, h the cascade's impulse response truncated at n."""
    s64 = np.asarray(s64, dtype=np.float64)
    e = EPS32 * np.abs(s64) * (1 + EPS32) + tol64_grid * scale(s64)
    h = np.abs(impulse_response(secs, len(s64)))
    return np.maximum(fftconvolve(h, e)[:len(s64)], 0.0) * (1 + 1e-12)


# ---- the deliberately wrong forms ---------------------------------------------------------------------------------------
def _f32_valued(secs):
    return [(np.asarray(b, dtype=np.float32).astype(np.float64), np.asarray(a, dtype=np.float32).astype(np.float64))
            for b, a in secs]


def wrong_forms(secs, x32, zi=None, initial=0.0):
    """name -> float32 rows: three host restatements of an IIR cascade that are NOT the double result rounded once
        f32_coefficients   the recurrence in double with every coefficient narrowed to float32
        f32_recurrence     the recurrence itself in float32 (its coefficients are float32 as well)
        round_per_section  double arithmetic, the row narrowed to float32 after EVERY section"""
    x64 = np.asarray(x32, dtype=np.float64)
    return {
        'f32_coefficients': iir_reference(_f32_valued(secs), x64, zi, initial)[0].astype(np.float32),
        'f32_recurrence': iir_reference(secs, np.asarray(x32, dtype=np.float32), zi, initial, dtype=np.float32)[0],
        'round_per_section': iir_reference(secs, x64, zi, initial, round_sections=True)[0].astype(np.float32),
    }


# ---- FIR --------------------------------------------------------------------------------------------------------------
FIR_L = 4096                   # fir_fused's transform length
FIR_KMAX = 1537                # taps one pass of it takes; longer kernels run as equal segments, accumulated


def fir_kernel(K, seed):
    ker = np.random.default_rng(seed).normal(size=K)
    return ker / np.abs(ker).sum()


def fir_reference(x32, kers):
    """the time-domain definition in double (the C oracle) on the widened rows; kers: (K,) or one kernel per row"""
    from oracle import c_oracle
    x64 = np.asarray(x32, dtype=np.float64)
    kers = np.broadcast_to(kers, (len(x64), np.shape(kers)[-1]))
    return np.stack([c_oracle.fir(row, np.ascontiguousarray(k)) for row, k in zip(x64, kers)])


def fir_host_f32(x32, ker):
    """One row through a SINGLE-PRECISION host restatement of the stage's algorithm: overlap-save with scipy.fft in
    float32 on windows of FIR_L samples, the kernel cut into equal segments of at most FIR_KMAX taps (each segment's
    spectrum formed in double and narrowed once, as the plan does), one pass per segment accumulated in float32.
        out[i] = sum_j sum_k' ker[j Kseg + k'] sig[(i + K//2 - j Kseg) - k']"""
    import scipy.fft
    x32 = np.asarray(x32, dtype=np.float32)
    n, K = len(x32), len(ker)
    nseg = -(-K // FIR_KMAX)
    Kseg = -(-K // nseg)
    hop = FIR_L - Kseg + 1
    out = np.zeros(n, dtype=np.float32)
    for j in range(nseg):
        seg = np.zeros(FIR_L)
        part = np.asarray(ker[j * Kseg:min(K, (j + 1) * Kseg)], dtype=np.float64)
        seg[:len(part)] = part
        H = np.fft.rfft(seg).astype(np.complex64)
        d = K // 2 - j * Kseg
        for i0 in range(0, n, hop):
            lo = i0 + d - (Kseg - 1)                              # the window's first input sample
            w = np.zeros(FIR_L, dtype=np.float32)
            a, b = max(lo, 0), min(lo + FIR_L, n)
            if b > a:
                w[a - lo:b - lo] = x32[a:b]
            y = scipy.fft.irfft(scipy.fft.rfft(w) * H, FIR_L)
            assert y.dtype == np.float32
            m = min(hop, n - i0)
            out[i0:i0 + m] += y[Kseg - 1:Kseg - 1 + m]
    return out


def fir_wrong_forms(x32, ker):
    """name -> float32 rows of an FIR that is not the double convolution rounded once: the single-precision transform
    above, and the double convolution with its TAPS narrowed to float32"""
    ker32 = np.asarray(ker, dtype=np.float32).astype(np.float64)
    return {
        'f32_transform': np.stack([fir_host_f32(row, ker) for row in x32]),
        'f32_taps': fir_reference(x32, ker32).astype(np.float32),
    }
