"""One NaN or +-Inf sample through the filter stages: how far it reaches, and that it reaches nothing else.

The rules are those of tests/nonfinite_ref.py (derived there, held to the host referees in tests/test_nonfinite_cpu.py,
stated per entry in include/wfk.h): the bad row is non-finite on all of the MINIMUM reach -- the outputs whose sum has a
term on the bad sample; a finite number there is a measurement that was never made -- and bit for bit the clean run
outside the MAXIMUM reach, the outputs computed in one transform with it; every other row is bit for bit the clean run.
`clean` is the same apply of the same plan on the same input without the bad sample, read back from the device.
"Bit for bit" or "non-finite", with the one exception below.

Three rows, the bad sample in the middle one; NaN, +Inf and -Inf; float64 and float32 (no stage here takes complex rows
on the device: complex signals are split into real rows on the host); out of place and, where the stage allows it, in
place.  Every case asserts the kernel name of the form it claims to hold, before AND after the applies: a data NaN is
not a time-out and must not flip a plan.  Each case prints the measured non-finite span against both reaches.

The sampled chains get their bad sample from the program: the middle channel carries a `samplingPoints` envelope with
one NaN (Inf) knot.  There `clean` is another plan (a finite knot compiles to other pieces), and two plans are not
promised equal bits: the bad row's non-finite set is held between the two reaches of the non-finite set of
`BatchSampler`'s own output for that channel, the other rows to the chain's existing bound of the oracle.

One exception to "bit for bit", found here and documented (include/wfk.h): the finite outputs of the single-pass IIR
depend on the order in which a row's chunks arrive, in the last bit.  Those forms are held, outside the reach, to
`nonfinite_ref.lookback_order_bound` -- what two clean applies may differ by, derived there -- see test_shared_cascade."""
import re

import numpy as np
import pytest
import torch
from scipy.signal import butter, lfilter

from cases import FP32_TOL, FP64_GRID_TOL, FP64_IIR_TOL
from nonfinite_ref import (assert_reach, fir_max_reach, fir_min_reach, fir_passes, iir_reach, lookback_order_bound,
                           nonfinite_span, reach_of_set, same_as_clean, whole_row_reach)
from oracle import c_oracle
from reflection_rows_ref import rows_input, transfer
from row_windows import bits_equal
import waveforms_amd as wf
from waveforms_amd import _engine, _flatten, distortion, workloads as wl
from waveforms_amd._sampling import BatchSampler
from waveforms_amd.distortion import exp_decay_filter

pytestmark = pytest.mark.gpu
BAD = {'nan': np.nan, '+inf': np.inf, '-inf': -np.inf}
DTYPES = {'double': (np.float64, torch.float64), 'float': (np.float32, torch.float32)}
ROWS, MID = 3, 1


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def rows_of(n, seed, tdt, rows=ROWS):
    """independent normal rows, row r times 10**(r % 3) (a row taken for another shows), as a device tensor"""
    x = np.random.default_rng(seed).normal(size=(rows, n)) * (10.0 ** (np.arange(rows) % 3))[:, None]
    return torch.from_numpy(x).to(dev(), tdt)


def poisoned(x, p, value, row=MID):
    xb = x.clone()
    xb[row, p] = value
    return xb


def sos_sections(*args):
    return [(r[:3], r[3:]) for r in butter(*args, output='sos')]


def set_env(monkeypatch, env, clear=()):
    for k in clear:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- FirStage (wfk_fir_apply) ------------------------------------------------------------------------------------
FIR_N = 20011            # more than five windows of the on-chip transform at K = 1024 (hop 3073)
FIR_ENV = ('WFK_FIR_ROCFFT', 'WFK_FIR_L', 'WFK_FIR_CHUNK')
FIR_CASES = {
    # form: (K, a kernel per row, environment, reach form, WFK_FIR_L, kernel name)
    'fused': (1024, False, {}, 'fused', None, 'fir_fused<{T}>'),
    'segments': (2401, False, {}, 'segments', None, 'fir_fused<{T}> x 2'),
    'rows': (64, True, {}, 'rows', None, 'fir_fused<{T}> per-row spectra'),
    # hop 992, 21 windows per row; chunks of two rows: rows 0 and 1 share one batched transform, row 2 is the tail plan
    'rocfft': (33, False, {'WFK_FIR_ROCFFT': '1', 'WFK_FIR_L': '1024', 'WFK_FIR_CHUNK': '2'}, 'rocfft', 1024,
               'fir_gather<{T}> + rocfft<L=1024,rows=2> + fir_multiply<{T}> + fir_scatter<{T}>'),
}


def fir_positions(n, K, form, L):
    """0 and n - 1, the first and last input sample of a window, the first sample of the second window of a pair, one in
    the middle of the row -- for the first and the last pass of the form"""
    ps = {0, n - 1, n // 2}
    for d, M, lead, _ in {fir_passes(n, K, form, L)[0], fir_passes(n, K, form, L)[-1]}:
        ps |= {2 * M - lead, 2 * M - lead + d - 1, 3 * M - lead, 3 * M - lead - 1}
    return sorted(p for p in ps if 0 <= p < n)


@pytest.mark.parametrize('T', list(DTYPES))
@pytest.mark.parametrize('form', list(FIR_CASES))
def test_fir_stage(form, T, monkeypatch):
    K, per_row, env, ref_form, L, name = FIR_CASES[form]
    dt, tdt = DTYPES[T]
    set_env(monkeypatch, env, FIR_ENV)
    n = FIR_N
    rng = np.random.default_rng(K)
    ker = rng.normal(size=(ROWS, K) if per_row else K)
    ker /= np.abs(ker).sum(axis=-1, keepdims=True)
    st = distortion.FirStage(ker, n, ROWS, dt)
    try:
        assert st.kernel_name() == name.format(T=T), st.kernel_name()
        x = rows_of(n, 10 + K, tdt)
        run = lambda xin: st.apply_torch(xin, torch.full_like(xin, 7.0)).cpu().numpy()
        clean = run(x)
        assert bits_equal(run(x), clean)                           # (what "bit for bit the clean run" stands on)
        for p in fir_positions(n, K, ref_form, L):
            for bad, value in BAD.items():
                lo, hi = fir_min_reach(n, K, p)
                span = assert_reach(run(poisoned(x, p, value)), clean, MID, lo, hi, *fir_max_reach(n, K, p, ref_form, L),
                                    f'FIR {form} K={K} {T} p={p} {bad}')
                assert span[2] >= hi - lo
        assert st.kernel_name() == name.format(T=T)
    finally:
        st.close()


# ---- the shared cascade (wfk_iir_apply) --------------------------------------------------------------------------
OP_CHUNK, OP_LB = 2048, 32         # csrc/wfk_iir.hip: a wave's chunk, a lane's run; the single pass starts at 4 * OP_CHUNK
IIR_N = 4 * OP_CHUNK + 37
IIR_ENV = ('WFK_IIR_ONEPASS', 'WFK_IIR_OP_DEPTH', 'WFK_IIR_SPIN', 'WFK_IIR_BIQ_CAP')
FOUR_FIRST_ORDER = [exp_decay_filter(A, tau, 2e9) for A, tau in ((0.03, 40e-9), (0.01, 900e-9), (-0.005, 20e-6), (0.02, 3e-7))]
IIR_CASES = {
    # form: (sections, environment, rows, n, kernel name).  The last template argument of iir_onepass says whether the
    # in-wave scan runs in plain double (fast poles: butter(4, 0.1)) or in double-double (slow poles: butter(4, 0.03))
    'three_launch': (sos_sections(4, 0.07), {'WFK_IIR_ONEPASS': '0'}, ROWS, IIR_N, 'iir_pass<{T},2,2>'),
    'onepass_butter_0.1': (sos_sections(4, 0.1), {}, ROWS, IIR_N, 'iir_onepass<{T},2,2,true>'),
    'onepass_butter_0.03': (sos_sections(4, 0.03), {}, ROWS, IIR_N, 'iir_onepass<{T},2,2,false>'),
    'first_order': (FOUR_FIRST_ORDER, {}, ROWS, IIR_N, 'iir_onepass<{T},4,1,true>'),
    'order3': ([butter(3, 0.05)], {}, ROWS, IIR_N, 'iir_onepass<{T},1,3,true>'),
    'cut': (sos_sections(6, 0.05), {}, ROWS, IIR_N, 'iir_onepass<{T},2,2,false> + iir_onepass<{T},1,2,true>'),
    'persistent': (sos_sections(4, 0.07), {}, 64, 200_003, 'iir_onepass<{T},2,2,false> persistent'),
}


def iir_positions(n, unit, run):
    """0, the last sample of a lane's run, the last sample of chunk (tile) 0 and the first of chunk 1, a sample of the
    ragged tail, n - 1"""
    return sorted({0, run - 1, unit - 1, unit, (n // unit) * unit + (n % unit) // 2, n - 1})


def check_iir_apply(st, x, clean, clean_zf, p, value, what, in_place, bad_row, apply_kw, own_state=None, order_bound=None):
    """one apply of an IirStage on x with `value` at (bad_row, p), against the clean apply: outputs by `assert_reach`,
    zf of the bad row non-finite in every state (`own_state(zf, r)`: the entries of row r's own sections), the other
    rows' zf bit for bit"""
    xb = poisoned(x, p, value, bad_row)
    zf = torch.full_like(clean_zf, 7.0)
    out = xb if in_place else torch.full_like(xb, 7.0)
    assert st.apply_torch(xb, out=out, zf=zf, **apply_kw) is out
    got, zf = out.cpu().numpy(), zf.cpu().numpy()
    lo, hi = iir_reach(x.shape[1], p)
    span = assert_reach(got, clean, bad_row, lo, hi, lo, hi, what, order_bound)
    assert span == (p, x.shape[1], x.shape[1] - p)
    own = zf[bad_row] if own_state is None else own_state(zf, bad_row)
    assert len(own) and not np.isfinite(own).any(), (what, 'zf of the bad row', zf[bad_row])
    czf = clean_zf.cpu().numpy()
    for r in range(x.shape[0]):
        if r != bad_row:
            msg = same_as_clean(zf[r], czf[r], None if order_bound is None else float(order_bound[r]))
            assert msg is None, (what, f'zf of row {r} changed', msg)


# What the `first_order` case found (four first-order sections, iir_onepass<double,4,1,true>, n = 8229): with the NaN in
# the ragged last chunk the bad row came back with sample 8192 -- the first of that chunk, before p = 8210 -- one ulp
# (2.22e-16) off the clean run.  Not the NaN's doing: 18 of 150 CLEAN applies of the plan on this input had that bit the
# other way.  The single pass closes a chunk's look-back on whichever earlier chunk has published a prefix, and the
# candidates are the same sum to rounding, not to the bit.  A look-back carried in double-double and rounded once removes
# it (1050 applies, one bit pattern) and costs 7-8 % of the kernel's time (256 x 1e7 fp64, same box: 9.48 -> 10.21 ms two
# biquads, 10.84 -> 11.59 ms four first-order sections): not kept.  The dependence is the documented behaviour
# (include/wfk.h) and the single-pass forms are held to `nonfinite_ref.lookback_order_bound` outside
# the reach -- bit for bit, or finite and within 72 double ulps of the row's peak -- instead of to the bit alone.
# (float rows under two biquads never take the persistent grid -- csrc/wfk_iir.hip, iir_op_shape -- so that form is double only)
@pytest.mark.parametrize('form,T', [(f, T) for f in IIR_CASES for T in DTYPES if (f, T) != ('persistent', 'float')])
def test_shared_cascade(form, T, monkeypatch):
    sections, env, rows, n, name = IIR_CASES[form]
    dt, tdt = DTYPES[T]
    set_env(monkeypatch, env, IIR_ENV)
    st = distortion.IirStage(sections, n, rows, dt)
    try:
        assert st.kernel_name() == name.format(T=T), st.kernel_name()
        bad_row = rows // 2
        x = rows_of(n, 20 + len(form), tdt, rows)
        zi = torch.from_numpy(np.random.default_rng(5).normal(size=(rows, st.state_dim)) * 0.1).to(dev())
        kw = dict(initial=0.25, zi=zi)
        clean_zf = torch.full((rows, st.state_dim), 7.0, dtype=torch.float64, device=dev())
        clean = st.apply_torch(x, out=torch.full_like(x, 7.0), zf=clean_zf, **kw).cpu().numpy()
        assert st.plan.status() is True
        # bit for bit in the three-launch form; the single pass is held to what two clean applies of it may differ by
        order = lookback_order_bound(clean, np.finfo(dt).eps) if 'iir_onepass<' in name else None
        # (persistent: 64 rows of 200 003 samples are 100 MB an apply -- every position and value in place, the form that
        #  tests/test_gpu_iir.py runs it in, and out of place with the NaN at every position; a chunk in the middle as well)
        few = form == 'persistent'
        ps = iir_positions(n, OP_CHUNK, OP_LB) + ([n // 2] if few else [])
        for p in ps:
            for bad, value in BAD.items():
                for in_place in ((False, True) if not few or bad == 'nan' else (True, )):
                    check_iir_apply(st, x, clean, clean_zf, p, value, f'IIR {form} {T} p={p} {bad} in_place={in_place}',
                                    in_place, bad_row, kw, order_bound=order)
                    assert st.plan.status() is True                # wfk_iir_status: WFK_OK, a data NaN is no time-out
                    assert st.kernel_name() == name.format(T=T), st.kernel_name()
    finally:
        st.close()


def underflow_distance(sections):
    """samples after which |pole|^d is 0.0 in double for EVERY pole of the cascade (so for the fastest one long before):
    2^-1075 rounds to zero, d > 1075 ln 2 / -ln max|pole|"""
    slowest = max(float(np.abs(np.roots(a)).max()) for _, a in sections)
    assert 0 < slowest < 1
    d = int(np.ceil(1075 * np.log(2) / -np.log(slowest))) + 1
    assert slowest ** d == 0.0
    return d


@pytest.mark.parametrize('form', ['single_pass', 'three_launch'])
def test_inf_stays_non_finite_after_the_transition_powers_underflow(form, monkeypatch):
    """butter(4, 0.4): every entry of the transition over the distance from the bad sample to the row's end is exactly
    0.0 in double.  A scan that carries states across chunks as U^k s must still say non-finite at the last sample
    (0 * Inf is NaN); one that skips a zero power says finite."""
    sections = sos_sections(4, 0.4)
    d = underflow_distance(sections)
    p = 100
    n = max(IIR_N, p + d + 2 * OP_CHUNK + 37)
    print(f'butter(4, 0.4): every pole power is 0.0 after {d} samples; n = {n}, bad sample at {p}')
    set_env(monkeypatch, {'WFK_IIR_ONEPASS': '0'} if form == 'three_launch' else {}, IIR_ENV)
    st = distortion.IirStage(sections, n, ROWS, np.float64)
    try:
        name = st.kernel_name()
        assert name.startswith('iir_pass<double,2,2>' if form == 'three_launch' else 'iir_onepass<double,2,2,'), name
        x = rows_of(n, 33, torch.float64)
        clean_zf = torch.full((ROWS, st.state_dim), 7.0, dtype=torch.float64, device=dev())
        clean = st.apply_torch(x, out=torch.full_like(x, 7.0), zf=clean_zf).cpu().numpy()
        for bad, value in BAD.items():
            check_iir_apply(st, x, clean, clean_zf, p, value, f'IIR long decay {form} {bad}', False, MID, {},
                            order_bound=None if form == 'three_launch' else lookback_order_bound(clean, np.finfo(np.float64).eps))
            assert st.plan.status() is True and st.kernel_name() == name
    finally:
        st.close()


# ---- IirStage per row (wfk_iir_rows_apply) -----------------------------------------------------------------------
TILE, LANE_RUN = 4096, 16          # csrc/wfk_iir_rows.hip: a workgroup's tile, 256 lanes x 16 samples
ROWS_N = 2 * TILE + 1037           # three tiles, the last one ragged
ROWS_SHAPES = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (3, 1), (4, 1), (2, 2)]      # SHAPES of tests/test_gpu_iir_rows.py


def random_rows(rng, batch, nsec, order):
    """per row: nsec sections of the given order, real poles in 0.3 .. 0.97, a[0] != 1 (tests/test_gpu_iir_rows.py)"""
    rows = []
    for _ in range(batch):
        secs = []
        for _ in range(nsec):
            a = np.poly(rng.uniform(0.3, 0.97, order) * rng.choice([-1, 1], order, p=[0.2, 0.8]))
            a0 = rng.uniform(0.5, 2.0)
            secs.append((rng.uniform(-1, 1, order + 1) * a0, a * a0))
        rows.append(secs)
    return rows


@pytest.mark.parametrize('T', list(DTYPES))
@pytest.mark.parametrize('nsec,order', ROWS_SHAPES)
def test_per_row_cascades(nsec, order, T):
    dt, tdt = DTYPES[T]
    n = ROWS_N
    rng = np.random.default_rng(100 * nsec + order)
    st = distortion.IirStage(random_rows(rng, ROWS, nsec, order), n, ROWS, dt)
    try:
        name = f'iir_rows_tile<{"f64" if T == "double" else "f32"},{nsec},{order}>'
        assert st.per_row and st.kernel_name() == name, st.kernel_name()
        x = rows_of(n, 40 + nsec + order, tdt)
        zi = torch.from_numpy(rng.normal(size=(ROWS, st.state_dim)) * 0.1).to(dev())
        kw = dict(initial=np.array([0.25, -0.5, 0.125]), zi=zi)
        clean_zf = torch.full((ROWS, st.state_dim), 7.0, dtype=torch.float64, device=dev())
        clean = st.apply_torch(x, out=torch.full_like(x, 7.0), zf=clean_zf, **kw).cpu().numpy()
        for p in iir_positions(n, TILE, LANE_RUN):
            for bad, value in BAD.items():
                for in_place in (False, True):
                    check_iir_apply(st, x, clean, clean_zf, p, value, f'IIR rows <{nsec},{order}> {T} p={p} {bad} in_place={in_place}',
                                    in_place, MID, kw, st.row_state)
        assert st.kernel_name() == name
    finally:
        st.close()


# ---- SpectralPlan and ReflectionStage: one transform per row -----------------------------------------------------
FS = 2e9
SPEC_TERMS = [('reflect', 0.21, 33.3e-9), ('correct', -0.12, 101e-9), ('delay', -7.7e-9)]
SPEC_N = (255, 4096, 10007)


def check_whole_rows(run, x, n, what):
    """run(x, in_place) -> host result; the bad row non-finite in every element, the others bit for bit"""
    clean = run(x, False)
    assert bits_equal(run(x, True), clean)
    for p in sorted({0, n // 2, n - 1}):
        for bad, value in BAD.items():
            for in_place in (False, True):
                lo, hi = whole_row_reach(n, p)
                span = assert_reach(run(poisoned(x, p, value), in_place), clean, MID, lo, hi, lo, hi,
                                    f'{what} p={p} {bad} in_place={in_place}')
                assert span == (0, n, n)


@pytest.mark.parametrize('T', list(DTYPES))
@pytest.mark.parametrize('n', SPEC_N)
def test_spectral_plan(n, T):
    dt, tdt = DTYPES[T]
    x = torch.from_numpy(rows_input(n, ROWS, 500 + n) * (10.0 ** np.arange(ROWS))[:, None]).to(dev(), tdt)
    H = torch.from_numpy(np.ascontiguousarray(transfer(SPEC_TERMS, np.fft.rfftfreq(n, 1 / FS)), dtype=np.complex128)).to(dev())
    plan = _engine.SpectralPlan(n, ROWS, dt)

    def run(xin, in_place):
        xin = xin.clone()
        out = xin if in_place else torch.full_like(xin, 7.0)
        plan.apply(xin.data_ptr(), out.data_ptr(), H.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
        return out.cpu().numpy()

    try:
        check_whole_rows(run, x, n, f'SpectralPlan n={n} {T}')
    finally:
        plan.close()


@pytest.mark.parametrize('T', list(DTYPES))
@pytest.mark.parametrize('n', SPEC_N)
def test_reflection_stage(n, T):
    dt, tdt = DTYPES[T]
    x = torch.from_numpy(rows_input(n, ROWS, 600 + n) * (10.0 ** np.arange(ROWS))[:, None]).to(dev(), tdt)
    # the bad row carries a product of all three kinds; one neighbour a single term, the other none (it passes unchanged)
    st = distortion.ReflectionStage([[('correct', 0.1, 3e-9)], SPEC_TERMS, []], n, FS, dt)

    def run(xin, in_place):
        xin = xin.clone()
        return st.apply_torch(xin, out=None if in_place else torch.full_like(xin, 7.0)).cpu().numpy()

    try:
        check_whole_rows(run, x, n, f'ReflectionStage n={n} {T}')
    finally:
        st.close()


# ---- sampled chains: the bad sample comes from the program -------------------------------------------------------
CHAIN_ENV = ('WFK_CHAIN_UNFUSED', )
KNOTS = 101


def chain_channels(fill, knot, n):
    """three channels on a grid of n samples; the middle one carries a `samplingPoints` envelope (a Hann window of 101
    knots over 30 ns in the middle of the grid) whose knot 50 is `knot` -- None: the window's own finite value"""
    env = np.hanning(KNOTS).copy()
    if knot is not None:
        env[KNOTS // 2] = knot
    if fill == 'awg':
        chans = [wl.awg_channel(wf, c, n, 2e9) for c in range(ROWS)]
        grid, at = wl.awg_grid(n, 2e9), 0.5 * n / 2e9
    else:
        chans = [wl.sum_channel(wf, 6, 1000 + c) for c in range(ROWS)]
        grid, at = ('linspace', 0.0, 6 * wl.SPAN, n, False), 3 * wl.SPAN
    chans[MID] = chans[MID] + (wf.samplingPoints(-wl.SPAN / 2, wl.SPAN / 2, env) >> at)
    return chans, grid


def sampler_bad_set(chans, grid, dt):
    """the non-finite set of BatchSampler's own output for the middle channel; the other channels are finite"""
    bs = BatchSampler(chans, grid)
    try:
        y = bs.to_host(dt)
    finally:
        bs.close()
    assert np.isfinite(y[[0, 2]]).all()
    bad = ~np.isfinite(y[MID])
    assert bad.any(), 'the bad knot reached no sample'
    return bad


def oracle_rows(chans, grid):
    return c_oracle.eval_grid(_flatten.flatten(chans), _flatten.grid_from_desc(grid))


def check_between(got_row, bad_in, rule_min, rule_max, what):
    got = ~np.isfinite(got_row)
    need, may = reach_of_set(bad_in, rule_min), reach_of_set(bad_in, rule_max)
    print(f'{what}: sampler non-finite on {nonfinite_span(np.where(bad_in, np.nan, 0.0))}, chain on {nonfinite_span(got_row)}; '
          f'minimum reach {int(need.sum())}, maximum reach {int(may.sum())} samples')
    assert not (need & ~got).any(), (what, 'FINITE inside the minimum reach, first at', int(np.flatnonzero(need & ~got)[0]))
    assert not (got & ~may).any(), (what, 'non-finite beyond the maximum reach, first at', int(np.flatnonzero(got & ~may)[0]))


def check_other_rows(got, want, tol, what):
    for r in (0, 2):
        assert np.isfinite(got[r]).all(), (what, r, nonfinite_span(got[r]))
        err = float(np.max(np.abs(got[r].astype(np.float64) - want[r])))
        bound = tol * max(1.0, float(np.abs(want[r]).max()))
        print(f'{what}: row {r} err {err:.3g} bound {bound:.3g}')
        assert err <= bound, (what, r, err, bound)


CHAIN_N = 20011
GENERAL = re.compile(r' \+ wfk_sample(_wide)?<')       # the general kernel (its float rows compute in double: _wide)
CHAIN_K = 1024
CHAIN_SECTIONS = FOUR_FIRST_ORDER[:2]
CHAIN_CASES = [(fill, unfused) for fill in ('awg', 'fine') for unfused in (False, True)]
# What the plans of these channels run (each asserted below).  A non-finite table value -- like a non-finite amplitude
# -- is never admitted to a fused group: the host compiler hands such a piece to the general kernel `wfk_sample<...>`,
# so the kernels that EVALUATE their input (fir_sampled, iir_sampled, iir_rows_sampled / _short) never see a non-finite
# sample of the program, and a chain over such a channel runs sampler -> stage.  The one fused form that does take it
# is fir_short at AWG rates: the general kernel writes the piece to the chain's workspace, the transform's workgroups
# copy it into their windows (hop 3072, the `sampled` geometry).


def chain_knots():
    return (('nan', np.nan), ('+inf', np.inf))


def cascade_rows(sections, x):
    """scipy, section after section, from rest, row by row -> (y, zf)"""
    ys, zfs = [], []
    for row in x:
        zf = []
        for b, a in sections:
            row, z = lfilter(b, a, row, zi=np.zeros(max(len(a), len(b)) - 1))
            zf.append(z)
        ys.append(row)
        zfs.append(np.concatenate(zf))
    return np.stack(ys), np.stack(zfs)


@pytest.mark.parametrize('T', list(DTYPES))
@pytest.mark.parametrize('fill,unfused', CHAIN_CASES)
def test_sampled_fir(fill, unfused, T, monkeypatch):
    dt, _ = DTYPES[T]
    set_env(monkeypatch, {'WFK_CHAIN_UNFUSED': '1'} if unfused else {}, CHAIN_ENV + FIR_ENV)
    n, K = CHAIN_N, CHAIN_K
    ker = np.random.default_rng(7).normal(size=K)
    ker /= np.abs(ker).sum()
    tol = FP64_GRID_TOL if T == 'double' else FP32_TOL
    for label, knot in (('clean', None), ) + chain_knots():
        chans, grid = chain_channels(fill, knot, n)
        sf = distortion.SampledFir(chans, grid, ker, dt)
        try:
            name = sf.plan.kernel_name()
            hybrid = fill == 'awg' and not unfused
            assert sf.fused == hybrid, (name, sf.why_not)
            if hybrid:
                assert name == f'wfk_sample<...> (pieces without a short form) + fir_short<{T},12>', name
            else:
                assert name.endswith(' + FIR') and (knot is None or GENERAL.search(name)), name
            got = sf.to_host()
            assert sf.plan.kernel_name() == name
        finally:
            sf.close()
        y = oracle_rows(chans, grid)
        want = {r: c_oracle.fir(y[r], ker) for r in (0, 2)}
        what = f'SampledFir {fill} {"unfused" if unfused else "default"} {T} {label} [{name}]'
        check_other_rows(got, want, tol, what)
        if knot is None:
            assert np.isfinite(got[MID]).all()
            continue
        form = 'sampled' if hybrid else 'fused'
        check_between(got[MID], sampler_bad_set(chans, grid, dt), lambda p: fir_min_reach(n, K, p),
                      lambda p: fir_max_reach(n, K, p, form), what)


@pytest.mark.parametrize('T', list(DTYPES))
@pytest.mark.parametrize('fill,unfused', CHAIN_CASES)
def test_sampled_iir(fill, unfused, T, monkeypatch):
    dt, tdt = DTYPES[T]
    set_env(monkeypatch, {'WFK_CHAIN_UNFUSED': '1'} if unfused else {}, CHAIN_ENV + IIR_ENV)
    n = CHAIN_N
    tol = FP64_IIR_TOL if T == 'double' else FP32_TOL
    for label, knot in (('clean', None), ) + chain_knots():
        chans, grid = chain_channels(fill, knot, n)
        si = distortion.SampledIir(chans, grid, CHAIN_SECTIONS, dtype=dt)
        try:
            name = si.plan.kernel_name()
            assert not si.fused and name.endswith(' + IIR') and (knot is None or GENERAL.search(name)), (name, si.why_not)
            out = torch.full((ROWS, n), 7.0, dtype=tdt, device=dev())
            zf = torch.full((ROWS, si.state_dim), 7.0, dtype=torch.float64, device=dev())
            si.launch_torch(out, zf=zf)
            assert si.plan.status() is True                        # a data NaN is no time-out ...
            assert si.plan.kernel_name() == name and not si.fused  # ... and the plan keeps its form
            got, zf = out.cpu().numpy(), zf.cpu().numpy()
        finally:
            si.close()
        want, wzf = cascade_rows(CHAIN_SECTIONS, oracle_rows(chans, grid)[[0, 2]])
        what = f'SampledIir {fill} {"unfused" if unfused else "default"} {T} {label} [{name}]'
        check_other_rows(got, {0: want[0], 2: want[1]}, tol, what)
        assert np.max(np.abs(zf[[0, 2]] - wzf)) <= tol * max(1.0, np.abs(wzf).max())
        if knot is None:
            assert np.isfinite(got[MID]).all() and np.isfinite(zf[MID]).all()
            continue
        check_between(got[MID], sampler_bad_set(chans, grid, dt), lambda p: iir_reach(n, p), lambda p: iir_reach(n, p), what)
        assert not np.isfinite(zf[MID]).any(), (what, zf[MID])


@pytest.mark.parametrize('T', list(DTYPES))
@pytest.mark.parametrize('fill,unfused', CHAIN_CASES)
def test_sampled_iir_rows(fill, unfused, T, monkeypatch):
    dt, tdt = DTYPES[T]
    set_env(monkeypatch, {'WFK_CHAIN_UNFUSED': '1'} if unfused else {}, CHAIN_ENV)
    n = CHAIN_N
    tol = FP64_IIR_TOL if T == 'double' else FP32_TOL
    sections_rows = [FOUR_FIRST_ORDER[:2], FOUR_FIRST_ORDER[2:], FOUR_FIRST_ORDER[1:3]]
    tile = f'iir_rows_tile<{"f64" if T == "double" else "f32"},2,1>'
    for label, knot in (('clean', None), ) + chain_knots():
        chans, grid = chain_channels(fill, knot, n)
        sr = distortion.SampledIirRows(chans, grid, sections_rows, dtype=dt)
        try:
            name = sr.kernel_name()
            assert not sr.fused and name.endswith(' + ' + tile) and (knot is None or GENERAL.search(name)), (name, sr.why_not)
            out = torch.full((ROWS, n), 7.0, dtype=tdt, device=dev())
            zf = torch.full((ROWS, sr.state_dim), 7.0, dtype=torch.float64, device=dev())
            sr.launch_torch(out, zf=zf)
            got, zf = out.cpu().numpy(), zf.cpu().numpy()
            assert sr.kernel_name() == name
        finally:
            sr.close()
        y = oracle_rows(chans, grid)
        what = f'SampledIirRows {fill} {"unfused" if unfused else "default"} {T} {label} [{name}]'
        want = {r: cascade_rows(sections_rows[r], y[r:r + 1]) for r in (0, 2)}
        check_other_rows(got, {r: want[r][0][0] for r in want}, tol, what)
        for r in want:
            assert np.max(np.abs(zf[r] - want[r][1][0])) <= tol * max(1.0, np.abs(want[r][1]).max())
        if knot is None:
            assert np.isfinite(got[MID]).all() and np.isfinite(zf[MID]).all()
            continue
        check_between(got[MID], sampler_bad_set(chans, grid, dt), lambda p: iir_reach(n, p), lambda p: iir_reach(n, p), what)
        assert not np.isfinite(zf[MID]).any(), (what, zf[MID])


def test_sampled_iir_with_a_fir_behind_the_cascade():
    """predistort(wav(t), filters, ker): the cascade loses [first bad sample, n), the FIR behind it reads that from
    K // 2 samples earlier on -- at most from the start of the block of the first window that reads the sample"""
    n, K = CHAIN_N, 64
    ker = np.random.default_rng(9).normal(size=K)
    ker /= np.abs(ker).sum()
    for label, knot in chain_knots():
        chans, grid = chain_channels('awg', knot, n)
        si = distortion.SampledIir(chans, grid, CHAIN_SECTIONS, ker=ker)
        try:
            name = si.plan.kernel_name()
            assert not si.fused and name.endswith(' + IIR + FIR') and GENERAL.search(name), (name, si.why_not)
            out = torch.full((ROWS, n), 7.0, dtype=torch.float64, device=dev())
            si.launch_torch(out)
            assert si.plan.status() is True and si.plan.kernel_name() == name
            got = out.cpu().numpy()
        finally:
            si.close()
        bad = sampler_bad_set(chans, grid, np.float64)
        after_iir = np.zeros(n, dtype=bool)
        after_iir[int(np.flatnonzero(bad)[0]):] = True
        what = f'SampledIir + FIR awg {label} [{name}]'
        check_between(got[MID], after_iir, lambda p: fir_min_reach(n, K, p), lambda p: fir_max_reach(n, K, p, 'fused'), what)
        want = cascade_rows(CHAIN_SECTIONS, oracle_rows(chans, grid)[[0, 2]])[0]
        check_other_rows(got, {0: c_oracle.fir(want[0], ker), 2: c_oracle.fir(want[1], ker)}, FP64_IIR_TOL, what)


# ---- the kernels that EVALUATE their input never see a non-finite value of the program ---------------------------
AMP_N = 4 * 16384 + 37             # four chunks of the fused scan in its longer (sweep) form: every chain can fuse


def amp_channels(amp):
    """three fusable channels of six pulses on a fine grid; the fourth pulse of the middle one is scaled by `amp` (the
    pieces keep their shapes: one more pulse of another kind would keep the scan from fusing whatever its amplitude)"""
    chans = [wl.sum_channel(wf, 6, 1000 + c) for c in range(ROWS)]
    ws = wl.pulses(wf, 6, 1000 + MID)
    ws[3] = amp * ws[3]
    chans[MID] = wl._tree_sum(ws)
    return chans, ('linspace', 0.0, 6 * wl.SPAN, AMP_N, False)


@pytest.mark.parametrize('T', list(DTYPES))
def test_a_non_finite_amplitude_falls_back_from_every_fused_chain(T, monkeypatch):
    """With a finite amplitude the three chains fuse (fir_sampled, iir_sampled, iir_rows_sampled: asserted).  With a NaN
    or Inf amplitude the host compiler hands the piece to the general kernel, so no chain over the channel fuses -- at a
    length at which it could -- and the bad samples take the reach of sampler -> stage; the other rows stay finite and
    inside the chain's bound of the oracle."""
    dt, tdt = DTYPES[T]
    set_env(monkeypatch, {}, CHAIN_ENV + FIR_ENV + IIR_ENV)
    n, K = AMP_N, 256              # (the time-domain oracle is n K products a row)
    ker = np.random.default_rng(7).normal(size=K)
    ker /= np.abs(ker).sum()
    sections_rows = [FOUR_FIRST_ORDER[:2], FOUR_FIRST_ORDER[2:], FOUR_FIRST_ORDER[1:3]]
    makers = {
        'SampledFir': (lambda ch, g: distortion.SampledFir(ch, g, ker, dt), f'fir_sampled<{T},12>', ' + FIR'),
        'SampledIir': (lambda ch, g: distortion.SampledIir(ch, g, CHAIN_SECTIONS, dtype=dt), f'iir_sampled<{T},2,1,', ' + IIR'),
        'SampledIirRows': (lambda ch, g: distortion.SampledIirRows(ch, g, sections_rows, dtype=dt),
                           f'iir_rows_sampled<{"f64" if T == "double" else "f32"},2,1>', ' + iir_rows_tile<'),
    }
    for label, amp in (('finite', 0.7), ('nan', np.nan), ('+inf', np.inf)):
        chans, grid = amp_channels(amp)
        y = oracle_rows(chans, grid)
        bad = None if label == 'finite' else sampler_bad_set(chans, grid, dt)
        for stage, (make, fused_name, unfused_part) in makers.items():
            plan = make(chans, grid)
            try:
                name = plan.kernel_name() if stage == 'SampledIirRows' else plan.plan.kernel_name()
                if label == 'finite':
                    assert plan.fused and name.startswith(fused_name), (stage, name, plan.why_not)
                else:
                    assert not plan.fused and unfused_part in name and GENERAL.search(name), (stage, name, plan.why_not)
                out = torch.full((ROWS, n), 7.0, dtype=tdt, device=dev())
                plan.launch_torch(out)
                torch.cuda.synchronize()
                if stage == 'SampledIir':
                    assert plan.plan.status() is True and plan.plan.kernel_name() == name
                got = out.cpu().numpy()
            finally:
                plan.close()
            what = f'{stage} amplitude {label} {T} [{name}]'
            if stage == 'SampledFir':
                want = {r: c_oracle.fir(y[r], ker) for r in (0, 2)}
                tol = FP64_GRID_TOL if T == 'double' else FP32_TOL
                rules = (lambda p: fir_min_reach(n, K, p), lambda p: fir_max_reach(n, K, p, 'fused'))
            else:
                secs = {0: CHAIN_SECTIONS, 2: CHAIN_SECTIONS} if stage == 'SampledIir' else {0: sections_rows[0], 2: sections_rows[2]}
                want = {r: cascade_rows(secs[r], y[r:r + 1])[0][0] for r in (0, 2)}
                tol = FP64_IIR_TOL if T == 'double' else FP32_TOL
                rules = (lambda p: iir_reach(n, p), lambda p: iir_reach(n, p))
            check_other_rows(got, want, tol, what)
            if bad is None:
                assert np.isfinite(got[MID]).all(), what
            else:
                check_between(got[MID], bad, *rules, what)
