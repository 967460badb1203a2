"""FFT-domain operations of distortion.py on the device, against
golden outputs of the real reference (tests/golden/spectral.npz).  The reference has no
tests for these functions: parity is pinned by reference-generated vectors only."""
import numpy as np
import pytest
import torch

import cases
import golden_io
from reflection_rows_ref import ref_row, rows_input, transfer
from waveforms_amd import _engine, distortion
import waveforms_amd as wf

pytestmark = pytest.mark.gpu
SPEC = golden_io.npz('spectral.npz')


@pytest.mark.parametrize('i', range(len(cases.spectral_cases())))
def test_reflection_and_shift(i):
    n, A, tau, fs = cases.spectral_cases()[i]
    sig = cases.spectral_input(i)
    scale = max(1.0, np.abs(sig).max())
    got = distortion.reflection(sig, A, tau, fs)
    assert np.max(np.abs(got - SPEC[f'{i}.refl'])) <= 1e-11 * scale
    # round trip: exact except for the Nyquist bin of an even-length signal, whose
    # imaginary part `.real` discards -- in the reference just the same (1.6e-7 here)
    back = distortion.correct_reflection(got, A, tau, fs)
    fr = np.fft.fftfreq(n, 1 / fs)
    Hf = distortion.reflection_filter(fr, A, tau)
    ref_back = np.fft.ifft(np.fft.fft(SPEC[f'{i}.refl']) / Hf).real
    assert np.max(np.abs(back - ref_back)) <= 1e-11 * scale
    assert np.max(np.abs(back - sig)) <= 1e-6 * scale
    corr = distortion.correct_reflection(sig, A, tau, fs)
    assert np.max(np.abs(corr - SPEC[f'{i}.corr'])) <= 1e-11 * scale
    sh = distortion.shift(sig, 3.3 / fs * (1 if i % 2 else -1), 1 / fs)
    assert np.max(np.abs(sh - SPEC[f'{i}.shift'])) <= 1e-12 * scale


def test_kernel_design_and_symbolic_branch():
    zk = distortion.zDistortKernel(1e-9, [(50e-9, 0.02), (400e-9, -0.01)])
    assert np.allclose(zk, SPEC['zker'], rtol=1e-12, atol=1e-15)
    w = wf.gaussian(10e-9) >> 20e-9
    c = distortion.correct_reflection(w, 0.1, 5e-9)
    assert isinstance(c, wf.Waveform)
    assert c == 1 / 0.9 * w - 0.1 / 0.9 * (w >> 5e-9)
    with pytest.raises(ValueError):
        distortion.correct_reflection(np.zeros(8), 0.1, 1e-9)


def test_shift_keeps_the_callers_dtype():
    # upstream is np.convolve(signal, ker, 'same') + an integer roll with np.zeros_like(signal)
    # (distortion.py:22-38): complex stays complex, integers stay integers when only whole samples move
    rng = np.random.default_rng(5)
    z = rng.normal(size=3001) + 1j * rng.normal(size=3001)
    for delay in (2.3, -4.7, 0.4):
        pts, delta = int(delay // 1.0), delay - int(delay // 1.0)
        want = np.convolve(z, np.array([0, 1 - delta, delta]), mode='same')
        if pts:
            r = np.zeros_like(want)
            if pts < 0:
                r[:pts] = want[-pts:]
            else:
                r[pts:] = want[:-pts]
            want = r
        got = distortion.shift(z, delay, 1.0)
        assert got.dtype == np.complex128 and np.max(np.abs(got - want)) <= 1e-13
    k = np.arange(10)
    got = distortion.shift(k, 3.0, 1.0)
    assert got.dtype == k.dtype and list(got) == [0, 0, 0, 0, 1, 2, 3, 4, 5, 6]


# --------------------------------------------------------------------------------------------------------------------
# wfk_spectral_plan as the public entry point it is (include/wfk.h): batches, where spec_mul broadcasts the one H over
# the rows with H[idx % nf]; the shortest rows; in place; a second H; a side stream; float32.  Straight through
# _engine.SpectralPlan on device buffers.  Reference per row: the reference's own ifft(fft(x) * H(fftfreq)).real
# (tests/reflection_rows_ref.py), one term list for all rows, H uploaded as transfer(terms, rfftfreq).  Bound per
# row: 1e-11 * max(1, max|x[r]|), the bound of this file.
# --------------------------------------------------------------------------------------------------------------------
FS = 2e9
TERMS = {'reflect': [('reflect', 0.21, 33.3e-9)],
         'product': [('reflect', 0.21, 33.3e-9), ('correct', -0.12, 101e-9), ('delay', -7.7e-9)]}
# batch * nf crosses a 256-thread block at a non-multiple in the last three: idx % nf off a block edge
BATCH_SHAPES = [(1, 1), (4, 1), (4, 2), (4, 3), (3, 255), (5, 256), (3, 10007), (2, 30000)]


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def h_of(terms, n):
    return transfer(terms, np.fft.rfftfreq(n, 1 / FS))


def run_plan(plan, x, H, in_place=False):
    """x (batch, n) NumPy, H (n // 2 + 1) complex128 -> the plan's result on torch's current stream"""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev())
    Hd = torch.from_numpy(np.ascontiguousarray(H, dtype=np.complex128)).to(dev())
    yd = xd if in_place else torch.full_like(xd, 7.0)
    plan.apply(xd.data_ptr(), yd.data_ptr(), Hd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    if not in_place:
        assert np.array_equal(xd.cpu().numpy(), x)             # the input is intact
    return yd.cpu().numpy()


def row_errors(got, x, terms):
    """(max error per row, bound per row) against the reference's formula"""
    want = np.stack([ref_row(row.astype(np.float64), terms, FS) for row in x])
    return (np.abs(got - want).max(axis=1), 1e-11 * np.maximum(1.0, np.abs(x).max(axis=1)))


@pytest.mark.parametrize('terms', list(TERMS))
@pytest.mark.parametrize('batch,n', BATCH_SHAPES)
def test_plan_batches_and_short_rows(batch, n, terms):
    x = rows_input(n, batch, 300 + n) * (10.0 ** (np.arange(batch) % 3))[:, None]
    plan = _engine.SpectralPlan(n, batch, np.float64)
    try:
        err, tol = row_errors(run_plan(plan, x, h_of(TERMS[terms], n)), x, TERMS[terms])
    finally:
        plan.close()
    print(f'batch {batch} n {n} {terms}: max err / bound per row ' + ' '.join(f'{e:.2g}/{t:.2g}' for e, t in zip(err, tol)))
    assert np.all(err <= tol)


@pytest.mark.parametrize('n', [1, 2, 3])
def test_transfer_host_short_signals(n):
    """distortion.reflection on 1, 2 and 3 samples; the reference returns x * H(0) = x for n = 1"""
    x = rows_input(n, 1, 320 + n)[0]
    got = distortion.reflection(x, 0.21, 33.3e-9, FS)
    assert got.shape == (n, )
    assert np.max(np.abs(got - ref_row(x, TERMS['reflect'], FS))) <= 1e-11 * max(1.0, np.abs(x).max())
    if n == 1:
        assert abs(got[0] - x[0]) <= 1e-11 * max(1.0, abs(x[0]))


@pytest.mark.parametrize('batch,n', [(3, 10007), (4, 2)])
def test_plan_in_place_is_out_of_place(batch, n):
    """out == in is allowed (wfk.h): the input is staged before anything is written.  Bitwise the same result."""
    x, H = rows_input(n, batch, 330 + n), h_of(TERMS['product'], n)
    plan = _engine.SpectralPlan(n, batch, np.float64)
    try:
        apart = run_plan(plan, x, H)
        inplace = run_plan(plan, x, H, in_place=True)
    finally:
        plan.close()
    err, tol = row_errors(apart, x, TERMS['product'])
    assert np.all(err <= tol)
    assert np.array_equal(apart, inplace)


def test_plan_second_h_and_side_stream():
    """the plan keeps nothing of an H: a second apply with another one gives the other one's result; and an apply on
    a side stream gives, bitwise, the default stream's"""
    batch, n = 3, 10007
    x = rows_input(n, batch, 340)
    plan = _engine.SpectralPlan(n, batch, np.float64)
    try:
        first = run_plan(plan, x, h_of(TERMS['reflect'], n))
        second = run_plan(plan, x, h_of(TERMS['product'], n))
        again = run_plan(plan, x, h_of(TERMS['reflect'], n))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = run_plan(plan, x, h_of(TERMS['product'], n))
        side.synchronize()
    finally:
        plan.close()
    for got, terms in ((first, 'reflect'), (second, 'product')):
        err, tol = row_errors(got, x, TERMS[terms])
        assert np.all(err <= tol), terms
    assert np.max(np.abs(first - second)) > 1e-3              # (the two H differ by far more than the bound)
    assert np.array_equal(again, first)
    assert np.array_equal(on_side, second)


@pytest.mark.parametrize('n', [255, 4096])
def test_plan_row_independence(n):
    """row r of a batch of 5 is bitwise the row run alone in a batch-1 plan, as
    test_gpu_reflection_rows.py::test_row_independence claims of the per-row stage"""
    batch = 5
    x, H = rows_input(n, batch, 350 + n), h_of(TERMS['product'], n)
    plan = _engine.SpectralPlan(n, batch, np.float64)
    one = _engine.SpectralPlan(n, 1, np.float64)
    try:
        together = run_plan(plan, x, H)
        alone = np.stack([run_plan(one, x[r:r + 1], H)[0] for r in range(batch)])
    finally:
        plan.close()
        one.close()
    for got in (together, alone):
        err, tol = row_errors(got, x, TERMS['product'])
        assert np.all(err <= tol)
    diff = np.abs(together - alone).max(axis=1)
    print(f'n {n}: batch of 5 against batch-1 plans, max |difference| per row ' + ' '.join(f'{d:.2g}' for d in diff))
    assert np.array_equal(together, alone)


@pytest.mark.parametrize('batch,n', [(3, 4096), (3, 10007)])
def test_plan_float32(batch, n):
    """float32 rows (H stays complex128) against the float64 reference.  No number is fixed: the bound is 8 times the
    error a single-precision HOST transform of the same rows makes against the same reference,
    scipy.fft.irfft(scipy.fft.rfft(x32) * H.astype(complex64), n).  The 8 allows rocFFT another factorisation at a
    prime length; a wrong bin or row misses it by orders of magnitude."""
    import scipy.fft
    terms = TERMS['product']
    x32 = rows_input(n, batch, 360 + n).astype(np.float32)
    H = h_of(terms, n)
    want = np.stack([ref_row(row.astype(np.float64), terms, FS) for row in x32])
    host = scipy.fft.irfft(scipy.fft.rfft(x32, axis=1) * H.astype(np.complex64)[None, :], n, axis=1)
    assert host.dtype == np.float32
    plan = _engine.SpectralPlan(n, batch, np.float32)
    try:
        got = run_plan(plan, x32, H)
    finally:
        plan.close()
    assert got.dtype == np.float32
    err_dev = float(np.abs(got.astype(np.float64) - want).max())
    err_host = float(np.abs(host.astype(np.float64) - want).max())
    print(f'float32 batch {batch} n {n}: device max err {err_dev:.3g}, single-precision host transform {err_host:.3g} '
          f'(scale {np.abs(x32).max():.3g})')
    assert err_host > 0 and err_dev <= 8 * err_host
