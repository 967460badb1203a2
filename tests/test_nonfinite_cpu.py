"""The reach rules of tests/nonfinite_ref.py against the host referees, and three wrong host forms that the shared
assertion must reject.  No device: the rules the GPU tests hold the kernels to are themselves held here to

  * oracle.c_oracle.fir, the time-domain definition: its NaN set is `fir_min_reach`;
  * a NumPy restatement of overlap-save with each form's window, hop, lead and pairing (np.fft per window, two windows
    packed as real and imaginary part where the device packs them): it reproduces c_oracle.fir on clean input -- so
    the geometry `fir_passes` read from the .hip files is the one that computes the FIR -- and its NaN set is
    `fir_max_reach`;
  * scipy.signal.lfilter, section after section, on five cascades: `iir_reach`."""
import numpy as np
import pytest
from scipy.signal import butter, lfilter

from nonfinite_ref import (FIR_FORMS, assert_reach, fir_max_reach, fir_min_reach, fir_passes, iir_reach, nonfinite_span,
                           reach_of_set, rocfft_window)
from oracle import c_oracle
from row_windows import bits_equal
from waveforms_amd.distortion import exp_decay_filter

pytestmark = pytest.mark.filterwarnings('ignore:invalid value encountered:RuntimeWarning')     # (Inf - Inf, 0 * Inf: the subject)
BAD = {'nan': np.nan, '+inf': np.inf, '-inf': -np.inf}
KS = (1, 2, 33, 1024, 1537, 2401)
N_FIR = 9001                      # three windows of the on-chip transform at K = 1024, a partial last one


def positions(n, K):
    return sorted({0, 1, K // 2, n // 2, n - 1} & set(range(n)))


def forms_of(K):
    """(form, WFK_FIR_L or None) that take a kernel of K taps"""
    out = [('fused' if K <= 1537 else 'segments', None), ('rows', None), ('rocfft', None)]
    two_k = 1
    while two_k < 2 * K:
        two_k *= 2
    out.append(('rocfft', max(two_k, 16)))                       # the shortest legal transform: hop L - K + 1 <= L / 2 + 1
    if K <= 1537:
        out.append(('sampled', None))
    return out


def overlap_save(x, ker, passes, zero_bad_windows=False):
    """Overlap-save as the device runs it, per row of x (rows, n): pass j convolves the taps [j Kseg, (j + 1) Kseg) with
    windows of L samples starting at b M - lead (zero padded), keeps outputs [Kseg - 1, Kseg - 1 + M) of each window
    as block b, and accumulates over the passes.  paired: windows 2q and 2q + 1 are the real and imaginary part of one
    complex transform.  zero_bad_windows: a WRONG form -- a window that holds a non-finite sample is replaced by zeros."""
    x = np.atleast_2d(x)
    rows, n = x.shape
    K, nseg = len(ker), len(passes)
    kseg = (K + nseg - 1) // nseg
    out = np.zeros((rows, n))
    for j, (L, M, lead, paired) in enumerate(passes):
        taps = np.zeros(L)
        seg = ker[j * kseg:min(K, (j + 1) * kseg)]
        taps[:len(seg)] = seg
        nblk = (n + M - 1) // M

        def window(r, b):
            idx = b * M - lead + np.arange(L)
            ok = (idx >= 0) & (idx < n)
            w = np.zeros(L)
            w[ok] = x[r, idx[ok]]
            return np.zeros(L) if zero_bad_windows and not np.isfinite(w).all() else w

        def put(r, b, vals):
            lo, hi = b * M, min(n, (b + 1) * M)
            if lo < hi:
                out[r, lo:hi] += vals[kseg - 1:kseg - 1 + hi - lo]

        for r in range(rows):
            if paired:
                H = np.fft.fft(taps)
                for q in range((nblk + 1) // 2):
                    z = np.fft.ifft(np.fft.fft(window(r, 2 * q) + 1j * window(r, 2 * q + 1)) * H)
                    put(r, 2 * q, z.real)
                    put(r, 2 * q + 1, z.imag)
            else:
                H = np.fft.rfft(taps)
                for b in range(nblk):
                    put(r, b, np.fft.irfft(np.fft.rfft(window(r, b)) * H, L))
    return out


def overlap_save_rows_packed(x, ker, passes):
    """A WRONG form: rows 2q and 2q + 1 of the batch packed into one complex transform, window by window (unpaired
    windows; an odd last row is packed with zeros).  On finite input it is as good as the right one."""
    rows, n = x.shape
    out = np.zeros((rows, n))
    (L, M, lead, _), = passes
    K = len(ker)
    H = np.fft.fft(np.r_[ker, np.zeros(L - K)])
    for r0 in range(0, rows, 2):
        for b in range((n + M - 1) // M):
            idx = b * M - lead + np.arange(L)
            ok = (idx >= 0) & (idx < n)
            w = np.zeros((2, L))
            for k in range(min(2, rows - r0)):
                w[k, ok] = x[r0 + k, idx[ok]]
            z = np.fft.ifft(np.fft.fft(w[0] + 1j * w[1]) * H)
            lo, hi = b * M, min(n, (b + 1) * M)
            for k, part in zip(range(min(2, rows - r0)), (z.real, z.imag)):
                out[r0 + k, lo:hi] = part[K - 1:K - 1 + hi - lo]
    return out


# ---- the FIR rules ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', KS)
def test_fir_min_reach_is_the_support_of_the_time_domain_sum(K):
    rng = np.random.default_rng(K)
    n = N_FIR
    x, ker = rng.normal(size=n), rng.normal(size=K)
    ker[K // 3] = 0.0                                             # (a zero tap shortens nothing: 0 * NaN is NaN)
    for p in positions(n, K):
        for bad in BAD.values():
            xb = x.copy()
            xb[p] = bad
            got = ~np.isfinite(c_oracle.fir(xb, ker))
            lo, hi = fir_min_reach(n, K, p)
            want = np.zeros(n, dtype=bool)
            want[lo:hi] = True
            assert np.array_equal(got, want), (K, p, bad, nonfinite_span(c_oracle.fir(xb, ker)), (lo, hi))
    clean = c_oracle.fir(x, ker)
    xb = x.copy()
    xb[n // 2] = np.nan
    lo, hi = fir_min_reach(n, K, n // 2)
    got = c_oracle.fir(xb, ker)
    assert bits_equal(got[:lo], clean[:lo]) and bits_equal(got[hi:], clean[hi:])


@pytest.mark.parametrize('K', KS)
def test_fir_min_reach_lies_inside_every_forms_max_reach(K):
    for n in (1, 17, 2560, 3073, N_FIR, 20011):
        for form, L in forms_of(K):
            for p in sorted({0, 1, K // 2, n // 2, n - 1, n // 3, (2 * n) // 3} & set(range(n))):
                lo, hi = fir_min_reach(n, K, p)
                mlo, mhi = fir_max_reach(n, K, p, form, L)
                assert 0 <= mlo <= lo < hi <= mhi <= n, (K, n, form, L, p, (lo, hi), (mlo, mhi))


@pytest.mark.parametrize('K', KS)
def test_fir_max_reach_is_the_nan_set_of_overlap_save(K):
    rng = np.random.default_rng(100 + K)
    n = N_FIR
    x, ker = rng.normal(size=n), rng.normal(size=K)
    want_clean = c_oracle.fir(x, ker)
    for form, L in forms_of(K):
        passes = fir_passes(n, K, form, L)
        clean = overlap_save(x, ker, passes)[0]
        # the geometry computes the FIR: a window start, hop or lead that is off by one sample misses this by O(1)
        assert np.max(np.abs(clean - want_clean)) <= 1e-11 * max(1.0, np.abs(want_clean).max()), (K, form, L)
        d, M, lead, paired = passes[0]
        edges = {2 * M - lead, 2 * M - lead + d - 1, 3 * M - lead, M - lead - 1}     # first / last sample of a window ...
        for p in sorted((set(positions(n, K)) | edges) & set(range(n))):
            for bad in BAD.values():
                xb = x.copy()
                xb[p] = bad
                got = ~np.isfinite(overlap_save(xb, ker, passes)[0])
                lo, hi = fir_max_reach(n, K, p, form, L)
                want = np.zeros(n, dtype=bool)
                want[lo:hi] = True
                assert np.array_equal(got, want), (K, form, L, p, bad, nonfinite_span(np.where(got, np.nan, 0.0)), (lo, hi))


def test_the_rocfft_window_follows_the_knob():
    assert rocfft_window(33) == 1024 and rocfft_window(1024) == 8192 and rocfft_window(129) == 2048
    assert rocfft_window(33, 256) == 256 and rocfft_window(33, 64) == 1024 and rocfft_window(33, 300) == 1024
    assert rocfft_window(512, 1024) == 1024 and rocfft_window(513, 1024) == 8192
    assert set(FIR_FORMS) == {'fused', 'segments', 'rows', 'rocfft', 'sampled'}


def test_reach_of_a_set_is_the_union():
    bad = np.zeros(100, dtype=bool)
    bad[[3, 50]] = True
    m = reach_of_set(bad, lambda p: fir_min_reach(100, 9, p))
    assert list(np.flatnonzero(m)) == list(range(0, 8)) + list(range(46, 55))


# ---- the IIR rule ------------------------------------------------------------------------------------------------
CASCADES = {
    'butter(4, 0.03) sos': lambda: [(r[:3], r[3:]) for r in butter(4, 0.03, output='sos')],
    'four first-order exp-decay sections': lambda: [exp_decay_filter(A, tau, 2e9) for A, tau in
                                                    ((0.03, 40e-9), (0.01, 900e-9), (-0.005, 20e-6), (0.02, 3e-7))],
    'butter(3, 0.05)': lambda: [butter(3, 0.05)],
    'butter(4, 0.08)': lambda: [butter(4, 0.08)],
    'butter(4, 0.4) sos': lambda: [(r[:3], r[3:]) for r in butter(4, 0.4, output='sos')],
}


def cascade(sections, x):
    """scipy, section after section, from rest -> (y, zf): the sections' final states back to back"""
    zf = []
    for b, a in sections:
        x, z = lfilter(b, a, x, zi=np.zeros(max(len(a), len(b)) - 1))
        zf.append(z)
    return x, np.concatenate(zf)


@pytest.mark.parametrize('name', list(CASCADES))
@pytest.mark.parametrize('bad', list(BAD))
def test_iir_reach_is_what_lfilter_does(name, bad):
    sections = CASCADES[name]()
    n, p = 20000, 7001
    x = np.random.default_rng(len(name)).normal(size=(3, n))
    xb = x.copy()
    xb[1, p] = BAD[bad]
    clean, got = (np.stack([cascade(sections, row)[0] for row in a]) for a in (x, xb))
    zf_clean, zf = (np.stack([cascade(sections, row)[1] for row in a]) for a in (x, xb))
    lo, hi = iir_reach(n, p)
    span = assert_reach(got, clean, 1, lo, hi, lo, hi, f'lfilter {name} {bad}')
    assert span == (p, n, n - p)
    assert not np.isfinite(zf[1]).any(), zf[1]
    assert bits_equal(zf[[0, 2]], zf_clean[[0, 2]])
    if bad == 'nan':
        assert np.isnan(got[1, p:]).all()
    else:
        assert (~np.isnan(got[1, p:])).sum() <= 2                    # (+-inf: NaN in all but one or two samples)


# ---- the assertion bites -----------------------------------------------------------------------------------------
def _three_rows(n, seed):
    x = np.random.default_rng(seed).normal(size=(3, n))
    xb = x.copy()
    return x, xb


def test_a_right_overlap_save_passes_the_assertion():
    n, K, p = N_FIR, 1024, 4000
    x, xb = _three_rows(n, 1)
    xb[1, p] = np.nan
    ker = np.random.default_rng(2).normal(size=K)
    passes = fir_passes(n, K, 'fused')
    span = assert_reach(overlap_save(xb, ker, passes), overlap_save(x, ker, passes), 1,
                        *fir_min_reach(n, K, p), *fir_max_reach(n, K, p, 'fused'), 'overlap-save')
    assert span[2] == 2 * (4096 - K + 1) or span[1] == n          # both blocks of the pair


def test_two_rows_in_one_transform_are_rejected():
    """rows 0 and 1 as x0 + i x1: fine on finite input, and row 1's NaN takes row 0 with it"""
    n, K, p = 5000, 33, 2500
    x, xb = _three_rows(n, 3)
    xb[1, p] = np.nan
    ker = np.random.default_rng(4).normal(size=K)
    passes = fir_passes(n, K, 'rocfft')
    clean, got = overlap_save_rows_packed(x, ker, passes), overlap_save_rows_packed(xb, ker, passes)
    want = np.stack([c_oracle.fir(row, ker) for row in x])
    assert np.max(np.abs(clean - want)) <= 1e-11 * np.abs(want).max()       # no tolerance would show it
    with pytest.raises(AssertionError, match='row 0 holds no bad sample'):
        assert_reach(got, clean, 1, *fir_min_reach(n, K, p), *fir_max_reach(n, K, p, 'rocfft'), 'rows packed')


def test_a_zeroed_window_is_rejected():
    """the bad window replaced by zeros: every output finite and plausible"""
    n, K, p = N_FIR, 1024, 4000
    x, xb = _three_rows(n, 5)
    ker = np.random.default_rng(6).normal(size=K)
    passes = fir_passes(n, K, 'fused')
    clean = overlap_save(x, ker, passes, zero_bad_windows=True)
    for bad in BAD.values():
        xb[1, p] = bad
        got = overlap_save(xb, ker, passes, zero_bad_windows=True)
        assert np.isfinite(got).all()
        with pytest.raises(AssertionError, match='FINITE at'):
            assert_reach(got, clean, 1, *fir_min_reach(n, K, p), *fir_max_reach(n, K, p, 'fused'), 'zeroed window')


def chunked_first_order(x, b0, pole, chunk, drop_underflow):
    """y[i] = b0 x[i] + pole y[i - 1] as a chunked scan: each chunk from a zero state, plus pole^(j + 1) times the state
    at its start.  drop_underflow: a WRONG form -- a term whose transition power has underflowed to zero is skipped
    ("it contributes nothing"), so a non-finite state is gone 1075 samples later."""
    x = np.atleast_2d(x)
    out = np.empty_like(x)
    powers = pole ** np.arange(1, chunk + 1)
    for r, row in enumerate(x):
        state = 0.0
        for c0 in range(0, len(row), chunk):
            seg = row[c0:c0 + chunk]
            local = lfilter([b0], [1.0, -pole], seg)
            pw = powers[:len(seg)]
            with np.errstate(invalid='ignore'):
                carried = np.where(pw == 0.0, 0.0, pw * state) if drop_underflow else pw * state
            out[r, c0:c0 + len(seg)] = local + carried
            state = out[r, c0 + len(seg) - 1]
    return out


def test_a_dropped_underflowed_state_is_rejected():
    """0.5^1075 == 0: after an Inf, the wrong form is finite again from sample 1075 of the next chunk on"""
    n, p, chunk, pole = 4 * 2048 + 37, 100, 2048, 0.5
    assert pole ** 1075 == 0.0 and pole ** 1074 > 0.0
    x, xb = _three_rows(n, 7)
    lo, hi = iir_reach(n, p)
    right_clean = chunked_first_order(x, 0.3, pole, chunk, False)
    want = np.stack([lfilter([0.3], [1.0, -pole], row) for row in x])
    assert np.max(np.abs(right_clean - want)) <= 1e-12
    wrong_clean = chunked_first_order(x, 0.3, pole, chunk, True)
    for bad in ('+inf', '-inf', 'nan'):
        xb[1, p] = BAD[bad]
        assert_reach(chunked_first_order(xb, 0.3, pole, chunk, False), right_clean, 1, lo, hi, lo, hi, f'chunked scan {bad}')
        with pytest.raises(AssertionError, match='FINITE at'):
            assert_reach(chunked_first_order(xb, 0.3, pole, chunk, True), wrong_clean, 1, lo, hi, lo, hi, f'dropped state {bad}')


def test_the_assertion_checks_its_own_arguments():
    a = np.zeros((3, 10))
    b = a.copy()
    b[1, 4:7] = np.nan
    assert assert_reach(b, a, 1, 4, 7, 4, 7, 'self') == (4, 7, 3)
    assert assert_reach(b, a, 1, 5, 6, 2, 9, 'self') == (4, 7, 3)
    with pytest.raises(AssertionError, match='differs from the clean run before'):
        assert_reach(b, a, 1, 5, 7, 5, 7, 'self')
    with pytest.raises(AssertionError, match='differs from the clean run behind'):
        assert_reach(b, a, 1, 4, 6, 4, 6, 'self')
    with pytest.raises(AssertionError, match='FINITE at'):
        assert_reach(b, a, 1, 3, 7, 3, 7, 'self')
    c = b.copy()
    c[2, 0] = -0.0                                                 # bit for bit: -0.0 is not 0.0
    with pytest.raises(AssertionError, match='row 2 holds no bad sample'):
        assert_reach(c, a, 1, 4, 7, 4, 7, 'self')
    with pytest.raises(AssertionError, match='clean run is not finite'):
        assert_reach(b, b, 1, 4, 7, 4, 7, 'self')
