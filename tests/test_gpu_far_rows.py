"""Every row stage on two rows MORE THAN 2^32 ELEMENTS APART (tests/row_windows.py: `FarWindow`; DESIGN.md, "The row
rule": any stride >= n).  tests/test_gpu_row_windows.py and the stages' own window tests hold the rule at a stride of
n + 37; tests/test_gpu_huge.py holds rows LONGER than 2^31.  Here the row stride is 2^32 + 37 elements, so a
`row * stride` that loses its upper half anywhere -- in a kernel, or in a host-side pitch -- addresses row 0 or a guard
instead of row 1 (tests/test_far_rows_cpu.py shows that it can address nothing else) and fails an assertion.

One table, `CASES`, drives the file: (stage, form, dtype, side).  `side` says which rows are far: `in_place`, `far_in`
(far input, near output) or `far_out` (near input, far output); the near side is an ordinary `Window`, as only one
`FarWindow` can be alive.  Each case holds the four things of tests/test_gpu_row_windows.py:
  (a) the result against the reference the stage's own test file uses, at that file's bound (imported, not restated);
  (b) the result BIT FOR BIT what the same plan gives with ordinary `Window`s on both sides -- except where `iir_onepass`
      or `iir_sampled` runs, whose look-back sums in the order chunks publish: 1e-12 of the peak (FP32_TOL for float rows);
  (c) every guard of the arena and of the near window untouched;
  (d) on an out-of-place apply, the input bit for bit what was put there.
and the kernel-name prefix wherever the stage has a `kernel_name()`.  n is the smallest at which the form runs, as the
stage's own file has it.  The module frees the arena when it is done; its last test holds it to that."""
import functools

import numpy as np
import pytest
import torch

import dac_rows_ref
import extract_rows_ref
import reflection_rows_ref as refl
import shift_rows_ref
import test_gpu_dac_rows as dac_file
import test_gpu_demod as demod_file
import test_gpu_extract_rows as extract_file
import test_gpu_iir_rows as iir_rows_file
import test_gpu_iir_rows_chain as chain_rows_file
import test_gpu_phase_curve as probe_file
import test_gpu_reflection_rows as refl_file
import test_gpu_row_windows as near
import test_gpu_shift_rows as shift_file
import waveforms_amd as wf
from cases import FP32_TOL, FP64_FIR_TOL, FP64_GRID_TOL, FP64_IIR_TOL
from oracle import c_oracle
from row_windows import FAR_STRIDE, FarWindow, Window, bits_equal, free_far_arena
from waveforms_amd import _engine, _flatten, distortion, workloads as wl
from waveforms_amd._sampling import BatchSampler
from waveforms_amd.distortion import SampledFir, SampledIir, SampledIirRows
from waveforms_amd.utils import Demodulator

pytestmark = pytest.mark.gpu
ROWS = 2
F64, F32, C64, I16 = np.float64, np.float32, np.complex64, np.int16
_env, _sync, _peak, _torch = near._env, near._sync, near._peak, near._torch
_memory = {}


@pytest.fixture(scope='module', autouse=True)
def far_arena():
    """what the device had reserved before the module; the arena goes back when the module is done"""
    torch.cuda.synchronize()
    _memory['before'] = torch.cuda.memory_reserved()
    yield
    free_far_arena()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('dtype', [F64, F32, C64, I16], ids=lambda d: np.dtype(d).name)
def test_the_far_window_sees_every_guard(dtype):
    """the referee itself: the rows sit where the geometry says, writing them leaves the guards intact, and ONE element
    written anywhere else -- first and last of the arena, either side of either row, where a 32-bit slip of row 1 lands
    past a short row 0, the far end of a scan slab -- is reported with its offset"""
    n = 15
    x = np.arange(1, 2 * n + 1).reshape(2, n).astype(dtype)
    w = FarWindow(n, dtype, x)
    es = np.dtype(dtype).itemsize
    assert (w.stride, w.ptr) == (FAR_STRIDE, w.arena.data_ptr() + 5 * es) and w.arena.numel() == 5 + FAR_STRIDE + n + 37
    assert w.win[1].data_ptr() - w.win[0].data_ptr() == FAR_STRIDE * es > 2**32
    assert bits_equal(w.host(), x)
    assert bits_equal(torch.stack([w.arena[5:5 + n], w.arena[5 + FAR_STRIDE:5 + FAR_STRIDE + n]]).cpu().numpy(), x)
    w.assert_holds(x)
    last = w.arena.numel() - 1
    for at in (0, 5 + n, 5 + 37, 2**29 // es - 1, 2**29 // es, 5 + FAR_STRIDE - 1, 5 + FAR_STRIDE + n, last):
        kept = w.arena[at].clone()
        w.arena[at] = 1                                   # (for complex64: 1 + 0j, both components change)
        msg = w.guards_intact()
        assert msg is not None and msg.startswith('1 guard elements written') and f'offsets [{at}]' in msg, (at, msg)
        w.arena[at] = kept
    assert w.guards_intact() is None
    w.arena[4] = 1
    with pytest.raises(AssertionError, match=r'1 guard elements written; first at arena offsets \[4\]'):
        w.assert_guards()
    w.arena[4] = kept
    w.assert_holds(x)
    if dtype is C64:                                      # the imaginary part alone
        torch.view_as_real(w.arena)[3, 1] = 0.0
        assert 'offsets [3]' in w.guards_intact()
    older = w
    w = FarWindow(n, dtype)                               # refilled: the rows hold the sentinel again, the older one is dead
    assert w.guards_intact() is None and not bits_equal(w.host(), x)
    with pytest.raises(AssertionError, match='a later FarWindow'):
        older.host()


def _hold(side, apply, x=None, n=None, dtype=F64, out_shape=None, out_dtype=None):
    """Run `apply(src, dst)` twice -- with the far side of `side` a FarWindow, then with ordinary Windows -- on rows
    holding x (ROWS, n) (None: a stage without input rows); src / dst are the holders (`.win`, `.ptr`, `.stride`),
    dst is src for `in_place`, src is None without x.  Holds (c) and (d) for both runs.
    -> (far result, near result, what apply returned for the far run, for the near run)"""
    out_rows, out_n = out_shape or (ROWS, n)
    out_dtype = out_dtype or dtype
    assert side in ('in_place', 'far_in', 'far_out') and (side == 'far_out' or x is not None)
    res = []
    for far in (True, False):
        if side == 'in_place':
            src = FarWindow(n, dtype, x) if far else Window(ROWS, n, dtype, x)
            dst = src
        elif side == 'far_in':
            src = FarWindow(n, dtype, x) if far else Window(ROWS, n, dtype, x)
            dst = Window(out_rows, out_n, out_dtype)
        else:
            assert out_rows == ROWS
            src = None if x is None else Window(ROWS, n, dtype, x)
            dst = FarWindow(out_n, out_dtype) if far else Window(ROWS, out_n, out_dtype)
        if far:
            assert max(h.stride for h in (src, dst) if h is not None) == FAR_STRIDE
        extra = apply(src, dst)
        _sync()
        got = dst.host()
        dst.assert_guards()                                                               # (c)
        if src is not None and src is not dst:
            src.assert_holds(x)                                                           # (d)
        res.append((got, extra))
    return res[0][0], res[1][0], res[0][1], res[1][1]


def _same(got, twin, bitwise=True, dtype=F64, pk=1.0):
    if bitwise:
        assert bits_equal(got, twin), 'far rows differ from the same plan on an ordinary window'      # (b)
    else:
        diff = np.max(np.abs(got.astype(np.float64) - twin))
        assert diff <= (1e-12 if np.dtype(dtype) == np.dtype(F64) else FP32_TOL) * pk, diff / pk


# ---- BatchSampler / Plan.launch: the seven routes -------------------------------------------------------------------------
def _route_channels(route):
    """the route's builder of tests/test_gpu_row_windows.py, two rows of it (a second one made where it builds one)"""
    chans = near.SAMPLER_ROUTES[route][0]()
    return chans[:ROWS] if len(chans) >= ROWS else [chans[0], 0.5 * chans[0] + 0.125]


@functools.lru_cache(maxsize=None)
def _route_reference(route):
    _, grid, t, _, _ = near.SAMPLER_ROUTES[route]
    prog = _flatten.flatten(_route_channels(route))
    ref = c_oracle.eval_grid(prog, _flatten.grid_from_desc(grid)) if t is None else c_oracle.eval_tlist(prog, t())
    ref.setflags(write=False)
    return ref


def run_sampler(form, dtype, side):
    route, mode = form.rsplit('-', 1)
    accumulate = mode == 'accumulate'
    _, grid, t, env, starts = near.SAMPLER_ROUTES[route]
    ref = _route_reference(route)
    known = (3.0 - 2.0j) if np.dtype(dtype).kind == 'c' else 3.0
    with _env(env):
        chans = _route_channels(route)
        plan = BatchSampler(chans, grid).plan if t is None else _engine.Plan(_flatten.flatten(chans), t=t())
        assert plan.kernel_name().startswith(starts), plan.kernel_name()
        assert plan.n_channels == ROWS
        code = _engine._KIND_OF[np.dtype(dtype)]

        def apply(src, dst):
            if accumulate:
                dst.put(known)
            plan.launch(dst.ptr, dst.stride, code, accumulate, _stream())

        got, twin, _, _ = _hold(side, apply, n=plan.n, dtype=dtype)
        plan.close()
    want = ref + known if accumulate else ref
    tol = FP64_GRID_TOL if np.dtype(dtype) == np.dtype(F64) else FP32_TOL
    assert np.max(np.abs(got - want)) <= tol * _peak(ref), np.max(np.abs(got - want))     # (a)
    _same(got, twin)


# ---- IirStage, one cascade for all rows ----------------------------------------------------------------------------------
def run_iir_shared(form, dtype, side):
    secs, _, n, env, starts, ends, bitwise, tol = near.IIR_CASES[form]
    rng = np.random.default_rng(len(form) + ROWS)
    x = (rng.normal(size=(ROWS, n)) + 0.3).astype(dtype)
    D = sum(max(len(b), len(a)) - 1 for b, a in secs)
    zi = rng.normal(size=(ROWS, D)) * 0.1
    want, wzf = near._iir_reference(secs, x.astype(np.float64), zi)
    with _env(env):
        st = distortion.IirStage(secs, n, ROWS, dtype)
        name = st.kernel_name()
        assert all(p.startswith(starts) for p in name.split(' + ')) and name.endswith(ends), name
        zid = _torch(zi) if D else None

        def apply(src, dst):
            zfd = torch.full((ROWS, D), float('nan'), dtype=torch.float64, device='cuda') if D else None
            out = None if dst is src else dst.win
            assert st.apply_torch(src.win, out=out, initial=near._INITIAL, zi=zid, zf=zfd) is dst.win
            _sync()
            return zfd.cpu().numpy() if D else np.zeros((ROWS, 0))

        got, twin, zf, zf_twin = _hold(side, apply, x, n, dtype)
        st.close()
    bound = FP32_TOL if dtype is F32 else tol
    pk, zpk = _peak(want), _peak(wzf) if D else 1.0
    assert np.max(np.abs(got - want)) <= bound * pk, np.max(np.abs(got - want)) / pk      # (a)
    if D:
        assert np.max(np.abs(zf - wzf)) <= bound * zpk, np.max(np.abs(zf - wzf)) / zpk
    _same(got, twin, bitwise, dtype, pk)
    if bitwise:
        assert bits_equal(zf, zf_twin)


# ---- IirStage, one cascade per row (iir_rows_tile) ------------------------------------------------------------------------
def _row_cascades():
    """two rows with DIFFERENT cascades (two sections and one) of tests/test_gpu_iir_rows.py, and their levels"""
    pick = iir_rows_file.CASCADE_ROWS[3:5]
    secs = [iir_rows_file._filters(np.asarray(p).reshape(-1), rate) for rate, p, _ in pick]
    return secs, np.array([c for _, _, c in pick])


def run_iir_rows(form, dtype, side):
    n = iir_rows_file.TILE + 1
    secs, initial = _row_cascades()
    rng = np.random.default_rng(41)
    x = (rng.standard_normal((ROWS, n)) + initial[:, None]).astype(dtype)
    kind = 'f64' if dtype is F64 else 'f32'
    if form == 'per_row':
        st = distortion.IirStage(secs, n, ROWS, dtype=dtype)
        assert st.per_row and st.kernel_name().startswith(f'iir_rows_tile<{kind}'), st.kernel_name()
        feed = x

        def apply(src, dst):
            zf = torch.full((ROWS, st.state_dim), float('nan'), dtype=torch.float64, device='cuda')
            assert st.apply_torch(src.win, out=None if dst is src else dst.win, initial=initial, zf=zf) is dst.win
            _sync()
            return zf.cpu().numpy()

        got, twin, zf, zf_twin = _hold(side, apply, x, n, dtype)
        assert bits_equal(zf, zf_twin)
        st.close()
    else:                                               # every row reads the same n samples: row stride 0 inside
        assert side == 'far_out'
        plan = _engine.IirRowsPlan(secs, n, dtype)
        assert plan.kernel_name().startswith(f'iir_rows_tile<{kind}'), plan.kernel_name()
        shared = _torch(x[0])
        feed = np.stack([x[0], x[0]])
        lv = _torch(initial)

        def apply(src, dst):
            plan.apply_shared_in(shared.data_ptr(), dst.ptr, dst.stride, None, None, lv.data_ptr(), _stream())

        got, twin, _, _ = _hold(side, apply, n=n, dtype=dtype)
        assert bits_equal(shared.cpu().numpy(), x[0])                                     # (d)
        plan.close()
    for r in range(ROWS):
        want, _ = chain_rows_file._cascade(secs[r], feed[r].astype(np.float64), initial[r])
        scale = iir_rows_file._scale(want)
        err = float(np.max(np.abs(got[r] - want)))
        assert err <= (1e-9 if dtype is F64 else FP32_TOL) * scale, (r, err / scale)      # (a)
    _same(got, twin)


# ---- SampledIirRows: both fills ------------------------------------------------------------------------------------------
def run_sampled_iir_rows(form, dtype, side):
    fill, n = form, 8193
    key = ('edge', fill)
    chans, grid, secs, ini, _ = chain_rows_file._config(key)
    sr = SampledIirRows(chans, _flatten.grid_slice(grid, 0, n), secs, dtype=dtype)
    chain_rows_file._fused(sr, fill)

    def apply(src, dst):
        sr.launch_torch(dst.win, initial=ini)

    got, twin, _, _ = _hold(side, apply, n=n, dtype=dtype)
    chain_rows_file._check_rows(sr, key, got, None, 0, n, tol=chain_rows_file.TOL if dtype is F64 else FP32_TOL)   # (a)
    sr.close()
    _same(got, twin)


# ---- SampledIir: iir_sampled, and sampler -> IIR in place on the rows -------------------------------------------------------
def run_sampled_iir(form, dtype, side):
    fused = form == 'fused'
    n, secs = 40961, near._sos(4, 0.1)
    chans = [wl.sum_channel(wf, 6, 1000 + c) for c in range(ROWS)]
    grid = ('linspace', 0.0, 6 * wl.SPAN, n, False)
    x = c_oracle.eval_grid(_flatten.flatten(chans), _flatten.grid_from_desc(grid))
    zi = np.random.default_rng(5).normal(size=(ROWS, 4)) * 0.1
    want, wzf = near._iir_reference(secs, x, zi)
    with _env({} if fused else {'WFK_CHAIN_UNFUSED': '1'}):
        si = SampledIir(chans, grid, secs)
    assert si.fused == fused, si.why_not
    name = si.plan.kernel_name()
    assert name.startswith('iir_sampled<double,2,2,true>' if fused else 'wfk_sample') and not name.endswith('+ FIR'), name
    zid = _torch(zi)

    def apply(src, dst):
        zfd = torch.full((ROWS, 4), float('nan'), dtype=torch.float64, device='cuda')
        si.launch_torch(dst.win, initial=near._INITIAL, zi=zid, zf=zfd)
        assert si.plan.status()
        return zfd.cpu().numpy()

    got, twin, zf, zf_twin = _hold(side, apply, n=n, dtype=F64)
    si.close()
    assert np.max(np.abs(got - want)) <= FP64_IIR_TOL * _peak(want)                       # (a)
    assert np.max(np.abs(zf - wzf)) <= FP64_IIR_TOL * _peak(wzf)
    _same(got, twin, False, F64, _peak(want))
    assert np.max(np.abs(zf - zf_twin)) <= 1e-12 * _peak(wzf)


# ---- SampledFir ----------------------------------------------------------------------------------------------------------
def run_sampled_fir(form, dtype, side):
    build, grid, env, starts = near.SAMPLED_FIR[form]
    chans, ker = build()[:ROWS], near._fir_kernel(1024, 7)
    with _env(env):
        sf = SampledFir(chans, grid, ker, dtype)
    name = sf.plan.kernel_name()
    elem = '' if form == 'unfused' else ('double,' if dtype is F64 else 'float,')
    assert sf.fused == (form != 'unfused') and name.startswith(starts + elem), (name, sf.why_not)
    y = c_oracle.eval_grid(_flatten.flatten(chans), _flatten.grid_from_desc(grid))
    want = np.stack([c_oracle.fir(row, ker) for row in y])

    def apply(src, dst):
        sf.launch_torch(dst.win)

    got, twin, _, _ = _hold(side, apply, n=sf.n, dtype=dtype)
    sf.close()
    assert np.max(np.abs(got - want)) <= (1e-12 if dtype is F64 else FP32_TOL)            # (a)
    _same(got, twin)


# ---- FirStage ------------------------------------------------------------------------------------------------------------
def run_fir(form, dtype, side):
    K, env = near.FIR_CASES[form]
    n = 20011
    rng = np.random.default_rng(K)
    ker = rng.normal(size=K)
    ker /= np.abs(ker).sum()
    x = rng.normal(size=(ROWS, n)).astype(dtype)
    want = np.stack([c_oracle.fir(row, ker) for row in x.astype(np.float64)])
    with _env(env):
        st = distortion.FirStage(ker, n, ROWS, dtype)

        def apply(src, dst):
            st.apply_torch(src.win, dst.win)

        got, twin, _, _ = _hold(side, apply, x, n, dtype)
        st.close()
    assert np.max(np.abs(got - want)) <= (FP64_FIR_TOL if dtype is F64 else 1e-5) * _peak(want)      # (a)
    _same(got, twin)


# ---- ReflectionStage and the raw SpectralRowsPlan: rocFFT behind staging copies with the rows' pitch --------------------------
def _reflection_case(n, dtype):
    fs = 2e9 if n == 4096 else 1e9                       # the pairing of tests/test_gpu_reflection_rows.py: SHAPES
    x = refl.rows_input(n, ROWS, 31 + n).astype(dtype)
    terms = refl.rows_terms(5, 32 + n)[2:4]              # a product of two and one of three terms
    want = refl.ref_rows(x.astype(np.float64), terms, fs)
    if dtype is F64:
        return fs, x, terms, want, 1e-11 * refl_file.scale_of(x)
    # float rows: the bound of test_fp32 -- twice what SpectralPlan(float32) with a host-built H is off on the same rows
    f = np.fft.rfftfreq(n, 1 / fs)
    base = 0.0
    plan = _engine.SpectralPlan(n, 1, F32)
    for r in range(ROWS):
        xin = _torch(x[r])
        y = torch.empty_like(xin)
        H = _torch(refl.transfer(terms[r], f))
        plan.apply(xin.data_ptr(), y.data_ptr(), H.data_ptr(), _stream())
        base = max(base, float(np.max(np.abs(y.cpu().numpy() - want[r]))))
    plan.close()
    assert base > 0
    return fs, x, terms, want, 2 * base


def run_reflection(form, dtype, side):
    n = int(form)
    fs, x, terms, want, bound = _reflection_case(n, dtype)
    st = distortion.ReflectionStage(terms, n, fs, dtype)

    def apply(src, dst):
        assert st.apply_torch(src.win, out=None if dst is src else dst.win).data_ptr() == dst.ptr

    got, twin, _, _ = _hold(side, apply, x, n, dtype)
    st.close()
    assert np.max(np.abs(got - want)) <= bound, (np.max(np.abs(got - want)), bound)       # (a)
    _same(got, twin)


def run_spectral_rows(form, dtype, side):
    n = 4096
    fs, x, terms, want, bound = _reflection_case(n, dtype)
    plan = _engine.SpectralRowsPlan(terms, n, fs, dtype)

    def apply(src, dst):
        plan.apply(src.ptr, src.stride, dst.ptr, dst.stride, _stream())

    got, twin, _, _ = _hold(side, apply, x, n, dtype)
    plan.close()
    assert np.max(np.abs(got - want)) <= bound, (np.max(np.abs(got - want)), bound)       # (a)
    _same(got, twin)


# ---- ShiftStage ----------------------------------------------------------------------------------------------------------
def run_shift(form, dtype, side):
    n = 4099
    x = shift_file.rows_input(ROWS, n, 400 + n, dtype)
    st = distortion.ShiftStage([3.0, -1.25], n, 1.0, dtype)       # a whole-sample delay and a fractional one
    assert st.kernel_name() == ('shift_rows<double>' if dtype is F64 else 'shift_rows<float>')
    assert st.deltas[0] == 0.0 and 0.0 < st.deltas[1] < 1.0
    want, B = shift_rows_ref.shift_rows_ref(x, st.points, st.deltas)

    def apply(src, dst):
        assert st.apply_torch(src.win, dst.win).data_ptr() == dst.ptr

    got, twin, _, _ = _hold(side, apply, x, n, dtype)
    st.close()
    shift_rows_ref.check(got, want, B, f'far shift {side}', shift_rows_ref.EPS32 if dtype is F32 else 0.0)      # (a)
    _same(got, twin)


# ---- KernelExtractor -----------------------------------------------------------------------------------------------------
# n = 1026, skip = 1: k = 1024.  Rows of a length tests/test_gpu_extract_rows.py has no seeds for; these are the first
# seeds >= n + 1000 r (the shared one: >= n) that pass ITS rule -- the referee's two legs agree to 1e-13 of scale, which
# `rows_ref` asserts again here.  A property of the referee alone; found on the host.
EXTRACT_N, EXTRACT_SKIP, EXTRACT_M = 1026, 1, 10
EXTRACT_SEEDS, EXTRACT_SHARED_SEED = [1026, 2026], 1026


def run_extract(form, dtype, side):
    n, skip, M = EXTRACT_N, EXTRACT_SKIP, EXTRACT_M
    k = n - 2 * skip
    shared = form == 'shared_far_sig_out'
    if shared:
        a, b0 = extract_rows_ref.make_input(n, EXTRACT_SHARED_SEED)
        b = np.stack([b0 * (10.0**(r % 3) * (1 + r / 4)) for r in range(ROWS)])
    else:
        a, b = extract_file.rows_input(n, ROWS, EXTRACT_SEEDS)
    bw = extract_file.bw_of(M)
    want = extract_rows_ref.rows_ref(a, b, extract_rows_ref.taps_of(extract_file.FS, bw), skip, (n, M))
    ex = distortion.KernelExtractor(n, ROWS, extract_file.FS, bw, skip, shared_input=shared)
    assert ex.kernel_name() == 'extract_ratio + extract_smooth' and ex.k == k == 1024
    ad = _torch(a)
    if form == 'far_ker':                                # near inputs, the kernel rows far
        bd = Window(ROWS, n, F64, b)

        def apply(src, dst):
            assert ex.apply_torch(ad, bd.win, dst.win).data_ptr() == dst.ptr

        got, twin, _, _ = _hold('far_out', apply, n=k, dtype=F64)
        bd.assert_holds(b)                                                                # (d)
    else:                                                # the measured rows far, the kernel rows near

        def apply(src, dst):
            assert ex.apply_torch(ad, src.win, dst.win).data_ptr() == dst.ptr

        got, twin, _, _ = _hold('far_in', apply, b, n, F64, out_shape=(ROWS, k))
    assert bits_equal(ad.cpu().numpy(), a)                                                # (d)
    ex.close()
    want.check(got, f'far extract {form}')                                                # (a)
    _same(got, twin)


# ---- DacStage ------------------------------------------------------------------------------------------------------------
def run_dac(form, dtype, side):
    n, k = 8193, 2 if form == 'interleave2' else 1       # 8192 codes are one workgroup's span
    x = dac_file.rows_input(ROWS, n, 400 + n, dtype)
    g, o = dac_file.gains_offsets(ROWS, 14)
    st = distortion.DacStage(g, n, offset=o, bits=14, shift=2, interleave=k, dtype=dtype)
    assert st.kernel_name(counts=True) == f'dac_rows_count<{dac_file.NAME_OF["f64" if dtype is F64 else "f32"]}>'
    want, want_counts = dac_rows_ref.dac_ref(x, g, o, 14, 2, k)

    def apply(src, dst):
        counts = torch.full((ROWS, 3), -77, dtype=torch.int64, device='cuda')
        assert st.apply_torch(src.win, dst.win, counts).data_ptr() == dst.ptr
        return counts.cpu().numpy()

    got, twin, counts, counts_twin = _hold(side, apply, x, n, dtype, out_shape=(ROWS // k, k * n), out_dtype=I16)
    st.close()
    dac_file.same(got, want, f'far dac codes {form} {side}')                              # (a)
    dac_file.same(counts, want_counts, f'far dac counts {form} {side}')
    assert want_counts[:, :2].min() > 0                                                   # both rows clip on both rails
    _same(got, twin)
    assert np.array_equal(counts, counts_twin)


# ---- Demodulator ---------------------------------------------------------------------------------------------------------
def run_demod(form, dtype, side):
    nf, N = 5, 1000
    rng = np.random.default_rng(2)
    e = demod_file.tones(rng, nf, N)
    x = demod_file.traces(rng, ROWS, N, dtype)
    dm = Demodulator.from_matrix(e, dtype)
    name = dm.kernel_name(ROWS)                          # (two shots of 1000 samples: split over the record, then reduced)
    assert name.startswith('demod_tile<%s,' % {F64: 'double', F32: 'float', I16: 'short'}[dtype]), name
    res = []
    for far in (True, False):
        src = FarWindow(N, dtype, x) if far else Window(ROWS, N, dtype, x)
        out = Window(ROWS, nf, np.complex128)            # the result stays near: it is complex128
        assert dm.apply_torch(src.win, out.win).data_ptr() == out.ptr
        _sync()
        res.append(out.host())
        out.assert_guards()                                                               # (c)
        src.assert_holds(x)                                                               # (c), (d)
    demod_file.assert_parity(res[0], x, e)                                                # (a)
    _same(res[0], res[1])


def test_demodulator_rows_past_2_pow_31_elements():
    """contiguous int16 traces whose LAST rows start past element 2^31: S = 2^19 + 3 shots of N = 4100 (4.3 GB), made
    on the device; rows on both sides of the 2^31st element, the ends and 64 random ones against host NumPy"""
    S, N, nf = 2**19 + 3, 4100, 8
    assert (S - 1) * N > 2**31 and (2**18 + 1) * N < 2**31 < (S - 1) * N
    rng = np.random.default_rng(1)
    e = demod_file.tones(rng, nf, N)
    gen = torch.Generator(device='cuda').manual_seed(7)
    xt = torch.randint(-32768, 32768, (S, N), dtype=torch.int16, device='cuda', generator=gen)
    dm = Demodulator.from_matrix(e, I16)
    assert dm.kernel_name(S).startswith('demod_tile<'), dm.kernel_name(S)
    got = dm.apply_torch(xt)
    cross = 2**31 // N                                   # the row that holds element 2^31
    rows = np.r_[0, 1, 2, 2**18 - 1, 2**18, 2**18 + 1, cross - 1, cross, cross + 1, S - 1, rng.choice(S, 64, replace=False)]
    idx = torch.from_numpy(rows).cuda()
    demod_file.assert_parity(got[idx].cpu().numpy(), xt[idx].cpu().numpy(), e)
    del xt, got


# ---- BoxProbePlan, the probe behind PhaseCurve ---------------------------------------------------------------------------
def run_probe(form, dtype, side):
    pp, c, n = 37, 18, 5000
    rng, tlist, t, gain = probe_file.probe_input(pp, c, n)
    y = rng.standard_normal((ROWS, n))
    plan = _engine.BoxProbePlan(tlist, t, pp, c, gain)
    assert plan.kernel_name() == 'boxprobe_wave'
    wants, tol = probe_file.probe_numpy(y, n, tlist, t, pp, c, gain)

    def apply(src, dst):
        plan.apply(src.ptr, ROWS, src.stride, dst.ptr, dst.stride, _stream())

    got, twin, _, _ = _hold(side, apply, y, n, F64, out_shape=(ROWS, len(t)))
    plan.close()
    for r in range(ROWS):
        assert np.isnan(got[r, -1]) and np.isnan(wants[r, -1])
        assert np.max(np.abs(got[r, :-1] - wants[r, :-1])) <= tol, (r, np.max(np.abs(got[r, :-1] - wants[r, :-1])), tol)   # (a)
    _same(got, twin)


# ---- the table ------------------------------------------------------------------------------------------------------------
RUN = {'sampler': run_sampler, 'iir_shared': run_iir_shared, 'iir_rows': run_iir_rows,
       'sampled_iir_rows': run_sampled_iir_rows, 'sampled_iir': run_sampled_iir, 'sampled_fir': run_sampled_fir,
       'fir': run_fir, 'reflection': run_reflection, 'spectral_rows': run_spectral_rows, 'shift': run_shift,
       'extract': run_extract, 'dac': run_dac, 'demod': run_demod, 'probe': run_probe}
REAL = (F64, F32)
CASES = (                                                # (stage, form, dtype, side)
    [('sampler', f'{route}-{mode}', kind, 'far_out') for route in sorted(near.SAMPLER_ROUTES)
     for kind in (F64, F32, C64) for mode in ('store', 'accumulate')]
    + [('iir_shared', form, d, side) for form in ('three_launch', 'single_pass', 'gain') for d in REAL
       for side in ('in_place', 'far_in', 'far_out')]
    + [('iir_rows', 'per_row', d, side) for d in REAL for side in ('in_place', 'far_out')]
    + [('iir_rows', 'shared_input', d, 'far_out') for d in REAL]
    + [('sampled_iir_rows', fill, F64, 'far_out') for fill in chain_rows_file.FILLS]
    + [('sampled_iir', form, F64, 'far_out') for form in ('fused', 'unfused')]
    + [('sampled_fir', form, d, 'far_out') for form in sorted(near.SAMPLED_FIR) for d in REAL]
    + [('fir', form, d, side) for form in sorted(near.FIR_CASES) for d in REAL for side in ('far_in', 'far_out')]
    + [('reflection', str(n), d, side) for n in (4096, 10007) for d in REAL for side in ('in_place', 'far_in', 'far_out')]
    + [('spectral_rows', 'raw', F64, 'in_place')]
    + [('shift', 'whole_and_fraction', d, side) for d in REAL for side in ('far_in', 'far_out')]
    + [('extract', form, F64, side) for form, side in (('far_sig_out', 'far_in'), ('far_ker', 'far_out'),
                                                      ('shared_far_sig_out', 'far_in'))]
    + [('dac', 'codes', d, side) for d in REAL for side in ('far_in', 'far_out')]
    + [('dac', 'interleave2', F64, 'far_in')]
    + [('demod', 'traces', d, 'far_in') for d in (F64, F32, I16)]
    + [('probe', 'boxprobe', F64, 'far_in')]
)


@pytest.mark.parametrize('stage,form,dtype,side', CASES, ids=[f'{s}-{f}-{np.dtype(d).name}-{side}' for s, f, d, side in CASES])
def test_far_rows(stage, form, dtype, side):
    RUN[stage](form, dtype, side)


def test_the_arena_goes_back_to_the_device():
    """the last test of the module: after `free_far_arena()` the device holds what it held before the module, to 1 GiB"""
    free_far_arena()
    torch.cuda.synchronize()
    after = torch.cuda.memory_reserved()
    print(f'reserved before the module {_memory["before"] / 2**30:.2f} GiB, after {after / 2**30:.2f} GiB; '
          f'peak allocated {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB')
    assert after <= _memory['before'] + 2**30, (after, _memory['before'])
