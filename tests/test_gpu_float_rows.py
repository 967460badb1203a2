"""Float rows against the double result rounded ONCE, element by element (tests/float_rows_ref.py has the bound and its
derivation, tests/test_float_rows_cpu.py shows what it rejects; DESIGN.md §4 has the table of float forms).

Class A -- the kernel widens each sample, computes in double and narrows once at the store -- is held to
`check(got32, want64, tol64)` with the fp64 bound the form's own test file holds double rows to: the shared-cascade IIR
plan in every execution form, the per-row IIR stage in its eight shapes, the wide sampler builds, and the AWG-rate
sampler -> per-row IIR chain (whose sampler part is rounded into the tile first: its derived allowance is added).

Class B does float arithmetic inside.  Only FirStage is held to something new here, by the convention of
tests/test_gpu_spectral.py::test_plan_float32: 8 x the error of a single-precision host restatement of the same algorithm
against the same referee, per row.  The general sampler build without generic terms (`wfk_sample<float,...>`) turned out
to be class B as well: it keeps FP32_TOL, and the test says so.

Class C -- cut cascades, whose kernel names are joined by ' + ' -- run their middle passes in place on the float `out`,
one rounding per pass: they are NOT in the derived bound and keep their existing tests (FP32_TOL)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import float_rows_ref as fr
from cases import (FP32_TOL, FP64_FIR_TOL, FP64_GRID_TOL, FP64_IIR_TOL, FP64_TLIST_FUSED_TOL)
import waveforms_amd as wf
from oracle import c_oracle
from test_gpu_row_windows import SAMPLER_ROUTES
from waveforms_amd import _engine, _flatten, distortion, workloads as wl
from waveforms_amd._sampling import BatchSampler
from waveforms_amd.distortion import SampledIirRows

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.update({k: v})


def _torch(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared arrays are read-only)


# ---- class A: one cascade for all rows -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shared_reference(case):
    """x32, zi and the float64 referee of a shared cascade, computed once for both applies -> (x32, zi, want, wzf)"""
    secs, rows, n = fr.SHARED_CASES[case][:3]
    x32 = fr.shared_input(rows, n)
    zi = fr.state_input(rows, sum(fr.orders_of(secs)))
    want, wzf = fr.iir_reference(secs, x32.astype(np.float64), zi, fr.INITIAL)
    for a in (zi, want, wzf):
        a.setflags(write=False)
    return x32, zi, want, wzf


@pytest.mark.parametrize('inplace', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('case', sorted(fr.SHARED_CASES))
def test_shared_cascade_float_rows_are_rounded_once(case, inplace):
    """IirStage(float32) with one cascade for all rows, `initial` = 0.25 and a non-zero zi, in every form that is ONE
    pass: iir_pass, iir_onepass (plain and persistent), iir_scale, and the shaped single sections of order 3 and 6.
    Read in csrc/wfk_iir.hip: every store is (T)(iir_step_t(c, (double)x - pre, z) + post) -- `initial` is added BEFORE
    the narrowing -- and the state, the coefficients and zi / zf are double.  The settled tail (the input's floor at
    1e-3 of the step, filtered about the 0.25 level) is held by the element-wise bound, which is 1e-10 of the row's peak
    there where FP32_TOL was 5e-5.  Beyond the bound, every row must be float32(referee) bit for bit wherever the referee decides it: a third of
    the elements at tol64 = 1e-11, mostly on the step -- in the tail half an ulp is 6e-11 of the peak, about tol64
    itself, and the share that is decided there is printed (1 %; none at 5e-10).  zf, a double computed from exactly
    widened samples, is held to the double rows' own bound."""
    import torch
    secs, rows, n, env, starts, ends, tol64 = fr.SHARED_CASES[case]
    x32, zi, want, wzf = _shared_reference(case)
    D = zi.shape[1]
    with _env(env):
        st = distortion.IirStage(secs, n, rows, np.float32)
        name = st.kernel_name()
        assert ' + ' not in name and name.startswith(starts) and name.endswith(ends), name
        xd = _torch(x32)
        out = xd if inplace else torch.full_like(xd, float('nan'))
        zfd = torch.full((rows, D), float('nan'), dtype=torch.float64, device='cuda') if D else None
        assert st.apply_torch(xd, out=None if inplace else out, initial=fr.INITIAL, zi=_torch(zi) if D else None, zf=zfd) is out
        torch.cuda.synchronize()
        assert st.kernel_name() == name, (name, st.kernel_name())     # (no look-back timeout switched the form)
        got = out.cpu().numpy()
        zf = zfd.cpu().numpy() if D else np.zeros((rows, 0))
        if not inplace:
            assert np.array_equal(xd.cpu().numpy(), x32)
        st.close()
    assert got.dtype == np.float32
    fr.check(got, want, tol64, f'{case} {name}')
    fr.check_exactly_rounded(got, want, tol64, f'{case} whole rows')
    fr.check_exactly_rounded(got[:, -2000:], want[:, -2000:], tol64, f'{case} settled tail', S=fr.row_scale(want))
    if D:
        zerr = float(np.max(np.abs(zf - wzf))) / fr.scale(wzf)
        print(f'{case}: zf {zerr:.3g} of its scale (tol64 {tol64:g})')
        assert zerr <= tol64, zerr


# ---- class A: one cascade per row ------------------------------------------------------------------------------------
@pytest.mark.parametrize('inplace', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('nsec,order', fr.ROW_SHAPES)
def test_per_row_cascade_float_rows_are_rounded_once(nsec, order, inplace):
    """iir_rows_tile<f32, NSEC, ORD> in its eight shapes: three rows, every row its own exp-decay constants and its own
    `initial`, a non-zero zi, two whole tiles and a ragged third.  Read in csrc/wfk_iir_rows_body.inc: the tile holds T,
    both sweeps read (double)my[i] - pre, and the store is (T)(iir_cascade_step(...) + pre)."""
    import torch
    n, D = fr.N_ROWS, nsec * order
    secs = fr.row_cascades(nsec, order)
    x32, zi = fr.shared_input(3, n), fr.state_input(3, D)
    st = distortion.IirStage(secs, n, 3, np.float32)
    assert st.per_row and st.kernel_name() == f'iir_rows_tile<f32,{nsec},{order}>' and st.state_dim == D, st.kernel_name()
    xd = _torch(x32)
    out = xd if inplace else torch.full_like(xd, float('nan'))
    zfd = torch.full((3, D), float('nan'), dtype=torch.float64, device='cuda')
    assert st.apply_torch(xd, out=None if inplace else out, initial=fr.ROW_INITIAL, zi=_torch(zi), zf=zfd) is out
    torch.cuda.synchronize()
    got, zf = out.cpu().numpy(), zfd.cpu().numpy()
    st.close()
    for r in range(3):
        want, wzf = fr.iir_reference(secs[r], x32[r:r + 1].astype(np.float64), zi[r:r + 1], float(fr.ROW_INITIAL[r]))
        fr.check(got[r:r + 1], want, fr.TOL64_ROWS, f'iir_rows_tile<f32,{nsec},{order}> row {r}')
        fr.check_exactly_rounded(got[r:r + 1], want, fr.TOL64_ROWS, f'row {r}')
        assert np.max(np.abs(zf[r] - wzf[0])) <= fr.TOL64_ROWS * fr.scale(wzf)


# ---- the sampler: the wide builds (class A) and the one route that is not ---------------------------------------------
# route of tests/test_gpu_row_windows.py::SAMPLER_ROUTES -> tol64, its tier's bound against the C oracle
WIDE_ROUTES = {'per_factor': FP64_GRID_TOL, 'libm': FP64_GRID_TOL, 'pointwise_grid': FP64_GRID_TOL,
               'time_list': FP64_TLIST_FUSED_TOL}


def _sampler_plan(route):
    build, grid, t, env, starts = SAMPLER_ROUTES[route]
    prog = _flatten.flatten(build())
    plan = BatchSampler(build(), grid).plan if t is None else _engine.Plan(prog, t=t())
    assert plan.kernel_name().startswith(starts), plan.kernel_name()
    if t is None:
        ref = c_oracle.eval_grid(prog, _flatten.grid_from_desc(grid), want_complex=True)
    else:
        ref = c_oracle.eval_tlist(prog, t(), want_complex=True)
    return plan, ref


def _launch(plan, kind):
    import torch
    out = torch.full((plan.n_channels, plan.n), float('nan'), dtype=getattr(torch, np.dtype(kind).name), device='cuda')
    plan.launch(out.data_ptr(), plan.n, _engine._KIND_OF[np.dtype(kind)], False, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _components(a, kind):
    return {'re': np.ascontiguousarray(a.real), 'im': np.ascontiguousarray(a.imag)} if np.dtype(kind).kind == 'c' \
        else {'re': np.ascontiguousarray(a.real)}


@pytest.mark.parametrize('kind', [np.float32, np.complex64], ids=['float32', 'complex64'])
@pytest.mark.parametrize('route', sorted(WIDE_ROUTES))
def test_wide_sampler_builds_are_rounded_once(route, kind):
    """Float / complex64 launches of plans with generic terms and of time lists run wfk_sample_wide: wfk_sample_body with
    T = double and E = float, whose only narrowing is store_tile's (E)v (csrc/wfk_kernels.hip).  Per component against
    the C oracle at the tier's own fp64 bound; the distance to the SAME plan's double launch rounded once is printed."""
    tol64 = WIDE_ROUTES[route]
    with _env(SAMPLER_ROUTES[route][3]):
        plan, ref = _sampler_plan(route)
        name = plan.kernel_name(kind)
        assert all(p.startswith('wfk_sample_wide<') for p in name.split(' + ')), name
        wide = np.complex128 if np.dtype(kind).kind == 'c' else np.float64
        got, own = _launch(plan, kind), _launch(plan, wide)
        plan.close()
    S = fr.scale(ref)
    want, own = _components(ref, kind), _components(own, kind)
    for c, g in _components(got, kind).items():
        once = own[c].astype(np.float32)
        print(f'{route} {np.dtype(kind).name} {c}: {int(np.sum(g != once))} of {g.size} elements differ from the plan\'s own '
              f'double launch rounded once, worst {float(np.max(np.abs(g.astype(np.float64) - once))):.3g}')
        fr.check(g, want[c], tol64, f'{route} {name} {c}', S=S)


@pytest.mark.parametrize('kind', [np.float32, np.complex64], ids=['float32', 'complex64'])
def test_general_build_without_generic_terms_is_float_arithmetic(kind):
    """Route `general` (fused groups only, lean kernel off) is NOT a wide build: csrc/wfk_pick.h takes the wide tier only
    for time lists and for plans with generic or direct terms, so its float launch is wfk_sample<float,...> with float
    accumulators and float phasor recurrences -- class B.  It keeps FP32_TOL; what it makes of the round-once bound is
    printed, not asserted."""
    with _env(SAMPLER_ROUTES['general'][3]):
        plan, ref = _sampler_plan('general')
        name = plan.kernel_name(kind)
        assert name.startswith('wfk_sample<float,'), name
        got = _launch(plan, kind)
        plan.close()
    S = fr.scale(ref)
    want = _components(ref, kind)
    for c, g in _components(got, kind).items():
        worst = fr.report(g, want[c], fr.round_once_bound(want[c], FP64_GRID_TOL, S))
        print(f'general {name} {c}: worst |diff| / round-once bound = {worst[0]:.3g}, worst |diff| / peak = '
              f'{float(np.max(np.abs(g - want[c]))) / S:.3g}')
        assert np.max(np.abs(g - want[c])) <= FP32_TOL * S


# ---- class A behind one rounding of its input: the AWG-rate sampler inside the per-row IIR stage -------------------------
def test_awg_rate_sampled_iir_rows_float():
    """iir_rows_short<f32,2,1>: 3 rows x 20000 at 2 GS/s, two first-order sections and a level per row.  Read in
    csrc/wfk_iir_rows_sampled.hip: the entry evaluation accumulates in double (`double acc[R]`) and writes
    (T)(acc + coff) into the tile, which the shared tile body then filters in double and narrows once -- the float row
    is float32(F64(float32(s64))).  Bound: round_once_bound(want, FP64_IIR_TOL) + |h| (*) (2^-24 |s64| +
    FP64_GRID_TOL peak(s64)), h the row's impulse response (float_rows_ref.chain_input_allowance)."""
    import torch
    n = fr.N_AWG
    chans = [wl.awg_channel(wf, c, n, fr.CHAIN_RATE) for c in range(3)]
    grid = _flatten.grid_from_desc(wl.awg_grid(n, fr.CHAIN_RATE))
    secs = fr.chain_cascades()
    s64 = c_oracle.eval_grid(_flatten.flatten(chans), grid)
    sr = SampledIirRows(chans, grid, secs, np.float32)
    assert sr.fused and sr.kernel_name() == 'iir_rows_short<f32,2,1>' and (sr.n, sr.n_channels) == (n, 3), \
        (sr.kernel_name(), sr.why_not)
    out = torch.full((3, n), float('nan'), dtype=torch.float32, device='cuda')
    sr.launch_torch(out, initial=fr.CHAIN_INITIAL)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    sr.close()
    for r in range(3):
        want, _ = fr.iir_reference(secs[r], s64[r:r + 1], None, float(fr.CHAIN_INITIAL[r]))
        extra = fr.chain_input_allowance(secs[r], s64[r], FP64_GRID_TOL)
        print(f'row {r}: the input allowance is at most {float(extra.max()):.3g} (peak of the row {np.abs(want).max():.3g})')
        fr.check(got[r:r + 1], want, FP64_IIR_TOL, f'iir_rows_short<f32,2,1> row {r}', extra[None, :])


# ---- class B: the FIR stage ---------------------------------------------------------------------------------------------
FIR_ROWS, FIR_N = 4, 20011
FIR_CASES = {       # name -> (taps, one kernel per row, environment)
    'one_segment': (1024, False, {}),
    'two_segments': (2401, False, {}),          # the accumulate path
    'kernel_per_row': (64, True, {}),
    'rocfft': (1024, False, {'WFK_FIR_ROCFFT': '1'}),
}


@functools.lru_cache(maxsize=None)
def _fir_reference(K, per_row):
    """kernels, the double referee and the single-precision host restatement -- shared by the cases of equal kernels"""
    x32 = fr.shared_input(FIR_ROWS, FIR_N)
    kers = np.stack([fr.fir_kernel(K, K + r) for r in range(FIR_ROWS)]) if per_row else fr.fir_kernel(K, K)
    want = fr.fir_reference(x32, kers)
    rows = np.broadcast_to(kers, (FIR_ROWS, K))
    host = np.stack([fr.fir_host_f32(x, k) for x, k in zip(x32, rows)])
    return x32, kers, want, host


@pytest.mark.parametrize('case', sorted(FIR_CASES))
def test_fir_stage_float_rows_against_a_single_precision_host(case):
    """FirStage(float32): fir_fused<float> transforms in cx<float>, the rocFFT pipeline in single precision -- float
    arithmetic by design, so the bound is not the rounded double result but 8 x what a single-precision HOST restatement
    of the same overlap-save makes of the same rows against the same double referee (float_rows_ref.fir_host_f32:
    scipy.fft in float32, windows of 4096, segments of at most 1537 taps accumulated in float), per row.  The 8 is the
    allowance tests/test_gpu_spectral.py::test_plan_float32 makes for another factorisation; no device number is fixed."""
    import torch
    K, per_row, env = FIR_CASES[case]
    x32, kers, want, host = _fir_reference(K, per_row)
    with _env(env):
        st = distortion.FirStage(kers, FIR_N, FIR_ROWS, np.float32)
        xd = _torch(x32)
        got = st.apply_torch(xd, torch.full_like(xd, float('nan'))).cpu().numpy()
        st.close()
    assert got.dtype == np.float32 and np.array_equal(xd.cpu().numpy(), x32)
    once = fr.round_once_bound(want, FP64_FIR_TOL)
    for r in range(FIR_ROWS):
        err_dev = float(np.abs(got[r].astype(np.float64) - want[r]).max())
        err_host = float(np.abs(host[r].astype(np.float64) - want[r]).max())
        print(f'FIR {case} row {r}: device max err {err_dev:.3g}, single-precision host {err_host:.3g} (peak '
              f'{np.abs(want[r]).max():.3g}); worst |diff| / round-once bound: device '
              f'{fr.report(got[r], want[r], once[r])[0]:.3g}, host {fr.report(host[r], want[r], once[r])[0]:.3g}')
        assert err_host > 0 and err_dev <= 8 * err_host, (case, r, err_dev, err_host)
