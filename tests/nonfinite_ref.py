"""How far one non-finite sample reaches through the filter stages (include/wfk.h states the same per entry; DESIGN.md
section 4 lists the forms).  A plain module like row_windows.py: no device import, so the rules themselves are tested
on the host (tests/test_nonfinite_cpu.py) and the device is then held to them (tests/test_gpu_nonfinite.py).

One NaN or +-Inf sits in sample p of one row.  Two sets of outputs of that row matter:

  the MINIMUM reach   outputs whose defining sum has a term on sample p.  A kernel that writes a finite number there has
                      turned a missing measurement into a plausible one.
  the MAXIMUM reach   outputs the stage's form is allowed to lose: it computes them in one transform with sample p.
                      Outside it the row is bit for bit what it is without the bad sample, and so is every other row.

Both are half-open intervals [lo, hi) of output indices; every rule below returns (lo, hi).

FIR.  out[i] = sum_k ker[k] sig[i + K//2 - k], k < K, zero padded (csrc/wfk_fir.hip:4).  The term on sample p has
i + K//2 - k = p, so
    fir_min_reach = [p - K//2, p - K//2 + K) cut to [0, n)
and a zero tap does not shorten it: 0 * NaN is NaN.  The device does not evaluate that sum: it transforms windows of L
samples, and a transform spreads one non-finite input over all of its outputs (a DFT output is a sum over every input,
x * NaN and x + NaN are NaN, Inf * 0 and Inf - Inf are NaN).  A window b of a pass reads samples [s_b, s_b + L),
s_b = b * M - lead, and yields the output block [b * M, (b + 1) * M) cut to [0, n); where two windows travel as the
real and imaginary part of ONE complex transform (z = x1 + i x2 times a complex spectrum mixes them) a bad window takes
its partner's block too.  So
    fir_max_reach = the union, over every pass and every window b of it that reads p, of the blocks of b and of b's partner.
Consecutive windows overlap and the passes of a segmented kernel are less than a hop apart, so the union is one interval.
`fir_passes` spells the geometry out per form, each number next to the source line it restates.

IIR.  A recurrence has no window: y[i] depends on x[0..i], so the reach is [p, n) both ways -- everything before p is
bit for bit the clean run, everything from p on is non-finite (scipy.signal.lfilter: NaN gives NaN throughout, +-Inf gives
NaN in all but one or two samples; hence "non-finite", not "NaN") -- and the whole final state zf of the row with it.
This holds however far the bad sample lies behind: a chunked scan that multiplies a non-finite state by a transition
power which has underflowed to zero gets Inf * 0 = NaN, not 0.

Whole-row transforms (wfk_spectral_apply, wfk_spectral_rows_apply): one transform per row, the reach is the row."""
import numpy as np

from row_windows import bits_equal

FUSED_L = 4096                     # csrc/wfk_fft4096.h: FL, the on-chip transform
FUSED_KMAX = FUSED_L - 2559        # csrc/wfk_fir.hip:197  KMAX = FL - 2559 = 1537 taps in one transform
FUSED_MAXSEG = 4                   # csrc/wfk_fir.hip:197  WFK_FIR_MAXSEG
FIR_FORMS = ('fused', 'segments', 'rows', 'rocfft', 'sampled')


def rocfft_window(K, L=None):
    """the transform length of the rocFFT pipeline: the power of two >= 8 K, at least 1024 (csrc/wfk_fir.hip:204-205),
    unless `L` (what WFK_FIR_L holds) is a power of two >= 2 K (csrc/wfk_fir.hip:206)"""
    d = 1024
    while d < 8 * K:
        d *= 2
    if L is not None and L >= 2 * K and L & (L - 1) == 0:
        d = int(L)
    return d


def fir_passes(n, K, form, L=None):
    """-> [(L, M, lead, paired), ...]: one entry per pass over the row -- transform length, hop = outputs per window,
    samples a window starts in front of its block, and whether windows 2q and 2q + 1 share one complex transform.

      fused     K <= 1537, one pass of fir_fused                                (csrc/wfk_fir_fused.hip)
      segments  K > 1537: nseg = ceil(K / 1537) <= 4 passes of Kseg = ceil(K / nseg) taps, pass j reads j * Kseg earlier
      rows      a kernel per row (wfk_fir_plan_create_rows): the same launches, a spectrum per row -- the same geometry
      rocfft    fir_gather / rocFFT / fir_multiply / fir_scatter, real transforms of one window each, never paired.
                `L`: the value of WFK_FIR_L.  WFK_FIR_CHUNK cuts the BATCH into chunks of rows, each with its own
                batched transform: it moves no window of a row, so it does not enter the reach
      sampled   fir_sampled / fir_short (csrc/wfk_fir_sampled.hip): the fused transform at a hop of 256 * HOPB samples"""
    n, K = int(n), int(K)
    if form in ('fused', 'segments', 'rows'):
        nseg = (K + FUSED_KMAX - 1) // FUSED_KMAX                      # wfk_fir.hip:198  nseg = (K + KMAX - 1) / KMAX
        kseg = (K + nseg - 1) // nseg                                  # wfk_fir.hip:199  Kseg = (K + nseg - 1) / nseg
        assert nseg <= FUSED_MAXSEG, 'beyond four segments the plan is the rocFFT pipeline'       # wfk_fir.hip:200
        assert (nseg == 1) == (form != 'segments') or form == 'rows', (K, form)
        M = FUSED_L - kseg + 1                                         # wfk_fir.hip:209  M = L - Kt + 1, L = FL
        lead = (kseg - 1) - K // 2                                     # wfk_fir.hip:209  lead = (Kt - 1) - K / 2
        # wfk_fir.hip:313  pass sg is launched with lead + sg * Kseg;  wfk_fir_fused.hip:39-40  b1 = 2 pair, b2 = b1 + 1
        return [(FUSED_L, M, lead + j * kseg, True) for j in range(nseg)]
    if form == 'rocfft':
        d = rocfft_window(K, L)
        # wfk_fir.hip:209  M = L - K + 1, lead = (K - 1) - K / 2;  fir_gather (wfk_fir.hip:42): src = b * M + i - lead
        return [(d, d - K + 1, (K - 1) - K // 2, False)]
    if form == 'sampled':
        assert K <= FUSED_KMAX
        hopb = 12 if K <= 1025 else 10                                 # wfk_fir_sampled.hip:554  hopb = K <= 1025 ? 12 : 10
        # wfk_fir_sampled.hip:104 / :298  s1 = 2 pair hop - lead, the second window hop samples on (:189 / :421);
        # wfk_fir.hip:155  lead = (K - 1) - K / 2;  outputs r < M = hop of each window (:208-211 / :439-442)
        return [(FUSED_L, 256 * hopb, (K - 1) - K // 2, True)]
    raise ValueError(form)


def fir_min_reach(n, K, p):
    """outputs of a row of n samples whose time-domain sum has a term on sample p: the support of c_oracle.fir"""
    n, K, p = int(n), int(K), int(p)
    return max(0, p - K // 2), min(n, p - K // 2 + K)


def fir_max_reach(n, K, p, form, L=None):
    """outputs the form may lose to a bad sample p: the blocks of every window that reads p, and of its pair partner"""
    n, K, p = int(n), int(K), int(p)
    lo, hi = n, 0
    for d, M, lead, paired in fir_passes(n, K, form, L):
        nblk = (n + M - 1) // M                                        # wfk_fir.hip:210  nblk = (n + M - 1) / M
        # window b reads [b M - lead, b M - lead + d):  b M <= p + lead  and  b M > p + lead - d
        first = max(0, -((-(p + lead - d + 1)) // M))
        last = min((p + lead) // M, (nblk - 1) | 1 if paired else nblk - 1)    # (an odd nblk: window nblk is a partner too)
        for b in range(first, last + 1):
            for w in ((b, b ^ 1) if paired else (b, )):
                if w * M < n:
                    lo, hi = min(lo, w * M), max(hi, min(n, (w + 1) * M))
    return (lo, hi) if lo < hi else (0, 0)


def reach_of_set(bad, rule):
    """the union of rule(p) -> (lo, hi) over the indices of a boolean mask `bad`, as a boolean mask of the same length"""
    out = np.zeros(len(bad), dtype=bool)
    for p in np.flatnonzero(bad):
        lo, hi = rule(int(p))
        out[lo:hi] = True
    return out


def iir_reach(n, p):
    """outputs of a recurrence that a bad sample p reaches: all from p on (and all of the row's final state)"""
    return int(p), int(n)


def whole_row_reach(n, p):
    """a transform over the whole row (SpectralPlan, ReflectionStage)"""
    return 0, int(n)


LOOKBACK_ROUNDINGS = 72


def lookback_order_bound(clean, dtype_eps):
    """What two clean applies of the single-pass IIR (iir_onepass, iir_sampled) may differ by, per row of `clean`.

    A chunk's start state is a sum over earlier chunks that closes on whichever of them has published its prefix when
    the wave looks (csrc/wfk_iir.hip, op_chunk_start): every choice is the same sum in another association.  One
    evaluation rounds at most 64 lane terms (each a double-double mat-vec rounded once), 6 levels of the butterfly that
    adds them and the published prefix: 71 roundings of half an ulp of the largest partial sum, so two evaluations are
    within LOOKBACK_ROUNDINGS = 72 ulps (double) of the largest state of each other.  The cascades these tests run have
    unit gain to within a small factor from state to output and from input to state (Butterworth low-passes, exp-decay
    corrections), so the bound is 72 * 2^-52 * max(1, max|row|) on the outputs; rows stored as float add the rounding of
    the store, one float ulp of the same peak.  Measured where it was found: ONE element one double ulp (2.2e-16) off,
    18 of 150 clean applies.  Five orders of magnitude below the bound the stage is held to against SciPy, so a wrong
    sample cannot hide under it."""
    peak = np.maximum(1.0, np.abs(np.asarray(clean, dtype=np.float64)).max(axis=1))
    return (LOOKBACK_ROUNDINGS * 2.0 ** -52 + (dtype_eps if dtype_eps > 2.0 ** -50 else 0.0)) * peak


def nonfinite_span(row):
    """(first, last + 1, count) of the non-finite elements of a 1-D array; (0, 0, 0) if all are finite"""
    bad = np.flatnonzero(~np.isfinite(row))
    return (int(bad[0]), int(bad[-1]) + 1, len(bad)) if len(bad) else (0, 0, 0)


def same_as_clean(got, clean, order_bound):
    """-> None if `got` is `clean` bit for bit -- or, where `order_bound` (an absolute bound) is given, finite wherever
    it is not and nowhere further than the bound from it --, else a message"""
    if bits_equal(got, clean):
        return None
    off = np.flatnonzero(got.view(np.uint8).reshape(len(got), -1) != clean.view(np.uint8).reshape(len(clean), -1)) // got.dtype.itemsize
    off = np.unique(off)
    with np.errstate(invalid='ignore'):
        d = np.abs(got[off].astype(np.float64) - clean[off].astype(np.float64))
    msg = (f'{len(off)} elements differ in bits, first {int(off[0])}, last {int(off[-1])}, {int((~np.isfinite(got[off])).sum())} of '
           f'them non-finite, largest |difference| {float(np.nanmax(d)) if np.isfinite(d).any() else float("nan"):.3g}')
    if order_bound is not None and np.isfinite(got[off]).all() and float(d.max()) <= order_bound:
        print(f'    (order of arrival: {msg}; bound {order_bound:.3g})')
        return None
    return msg + ('' if order_bound is None else f'; bound {order_bound:.3g}')


def assert_reach(got, clean, rows_bad, lo_min, hi_min, lo_max, hi_max, what, order_bound=None):
    """`got`, `clean`: (rows, n) host arrays of one dtype -- the same apply of the same plan on the same input with and
    without the bad sample, both read back from the device.  Row `rows_bad` (an index, or several) is non-finite on all of
    [lo_min, hi_min) and bit for bit `clean` outside [lo_max, hi_max); every other row is bit for bit `clean`.
    Prints the measured span per bad row and returns it, (first, last + 1, count), for the first of them.

    `order_bound`: one absolute bound per row, ONLY for a form whose finite outputs are documented to depend on an order
    of arrival (the single-pass IIR: `lookback_order_bound`).  "Bit for bit `clean`" then reads: bit for bit, or finite
    and within the row's bound of it -- what two clean applies of that form may differ by; a NaN, an Inf or a plausible
    wrong number outside the reach fails as before."""
    got, clean = np.asarray(got), np.asarray(clean)
    assert got.shape == clean.shape and got.dtype == clean.dtype and got.ndim == 2, (what, got.shape, clean.shape)
    rows, n = got.shape
    bad_rows = [int(rows_bad)] if np.ndim(rows_bad) == 0 else [int(r) for r in rows_bad]
    assert 0 <= lo_max <= lo_min <= hi_min <= hi_max <= n, (what, lo_min, hi_min, lo_max, hi_max, n)
    assert np.isfinite(clean).all(), f'{what}: the clean run is not finite'
    first_span = None
    for r in range(rows):
        bound = None if order_bound is None else float(np.broadcast_to(order_bound, (rows, ))[r])
        if r not in bad_rows:
            msg = same_as_clean(got[r], clean[r], bound)
            if msg:
                raise AssertionError(f'{what}: row {r} holds no bad sample and differs from the clean run: {msg}')
            continue
        span = nonfinite_span(got[r])
        print(f'{what}: row {r} non-finite on [{span[0]}, {span[1]}), {span[2]} samples; minimum reach '
              f'[{lo_min}, {hi_min}) = {hi_min - lo_min}, maximum reach [{lo_max}, {hi_max}) = {hi_max - lo_max}')
        first_span = first_span or span
        fin = np.flatnonzero(np.isfinite(got[r, lo_min:hi_min]))
        assert len(fin) == 0, (f'{what}: row {r} is FINITE at {len(fin)} outputs of the minimum reach [{lo_min}, {hi_min}), '
                               f'first {lo_min + int(fin[0])}: {got[r, lo_min + int(fin[0])]!r}')
        for a, b, side in ((0, lo_max, 'before'), (hi_max, n, 'behind')):
            msg = same_as_clean(got[r, a:b], clean[r, a:b], bound)
            if msg:
                raise AssertionError(f'{what}: row {r} differs from the clean run {side} the maximum reach [{lo_max}, {hi_max}): '
                                     f'non-finite span {span}; from element {a}: {msg}')
    return first_span
