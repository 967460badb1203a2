"""Per-row reflection / inverse reflection / delay with the transfer function formed on the device
(distortion.ReflectionStage, csrc/wfk_spectral_rows.hip) against the reference's own formula applied row by row:
ifft(fft(x) * H(fftfreq(n, 1/fs))).real with H the product of the row's terms (tests/reflection_rows_ref.py).

Bound: 1e-11 * max(1, max|x|) per element, the bound tests/test_gpu_spectral.py holds the single-row path to.  A CPU
emulation of the device arithmetic (phase product in long double, reduced, then irfft(rfft * H)) stays below 4e-14 of
scale against that formula on every shape below, so the bound leaves two orders for rocFFT's own rounding."""
import numpy as np
import pytest
import torch

from reflection_rows_ref import random_term, ref_row, ref_rows, rows_input, rows_terms, transfer
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu
ROWS = 5
SHAPES = [(1, 1e9), (2, 2e9), (3, 1e9), (255, 2e9), (256, 1e9), (4096, 2e9), (10007, 1e9), (30000, 2e9)]


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def scale_of(x):
    return max(1.0, float(np.abs(x).max()))


def run_stage(x, terms_rows, fs, dtype=np.float64):
    """x (rows, n) NumPy -> the stage's result, in place on a contiguous device copy"""
    st = distortion.ReflectionStage(terms_rows, x.shape[1], fs, dtype)
    try:
        return st.apply_torch(torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev())).cpu().numpy()
    finally:
        st.close()


@pytest.mark.parametrize('i', range(len(SHAPES)))
def test_parity(i):
    n, fs = SHAPES[i]
    x, terms = rows_input(n, ROWS, 100 + i), rows_terms(ROWS, 200 + i)
    assert [len(t) for t in terms] == [0, 1, 2, 3, 0]
    got = run_stage(x, terms, fs)
    err = np.max(np.abs(got - ref_rows(x, terms, fs)))
    print(f'n={n} fs={fs:g}: max err {err:.3g} (scale {scale_of(x):.3g})')
    assert err <= 1e-11 * scale_of(x)


def test_term_cap_and_refused_amplitudes():
    n, fs = 4096, 2e9
    rng = np.random.default_rng(7)
    full = [random_term(rng) for _ in range(_engine.SPEC_ROWS_MAX_TERMS)]
    x = rows_input(n, 1, 8)
    err = np.max(np.abs(run_stage(x, [full], fs)[0] - ref_row(x[0], full, fs)))
    print(f'{len(full)} terms: max err {err:.3g}')
    assert err <= 1e-11 * scale_of(x)
    with pytest.raises(ValueError):
        distortion.ReflectionStage([full + [('delay', 1e-9)]], n, fs)
    for A in (1.0, 1.5, -1.0, -2.0):
        for kind in ('reflect', 'correct'):
            with pytest.raises(ValueError):
                distortion.ReflectionStage([[(kind, A, 10e-9)]], n, fs)


@pytest.mark.parametrize('n', [255, 4096])
def test_row_independence(n):
    """a row's result is bitwise the same alone, first and last in a batch whose other rows (signals, numbers of terms,
    terms) differ: the term table is indexed by the row and nothing else"""
    fs = 2e9
    rng = np.random.default_rng(11)
    mine = [('reflect', 0.21, 33.3e-9), ('delay', -7.7e-9), ('correct', -0.12, 101e-9)]
    x = rows_input(n, 1, 12)
    others_x, others_t = rows_input(n, 4, 13), [[random_term(rng) for _ in range(k)] for k in (1, 0, 8, 2)]
    alone = run_stage(x, [mine], fs)[0]
    first = run_stage(np.vstack([x, others_x]), [mine] + others_t, fs)[0]
    last = run_stage(np.vstack([others_x, x]), others_t + [mine], fs)[4]
    assert np.array_equal(alone, first) and np.array_equal(alone, last)
    assert np.max(np.abs(alone - ref_row(x[0], mine, fs))) <= 1e-11 * scale_of(x)


@pytest.mark.parametrize('n', [4096, 10007])
def test_agreement_with_the_single_row_path(n):
    """the same second transform, only H's rounding differs: host NumPy there, formed on the device here"""
    fs = 1e9
    rng = np.random.default_rng(21)
    x = rows_input(n, ROWS, 22)
    A, tau = rng.uniform(-0.3, 0.3, ROWS), rng.uniform(0, 200e-9, ROWS)
    got = run_stage(x, [[('reflect', a, t)] for a, t in zip(A, tau)], fs)
    want = np.stack([distortion.reflection(x[r], A[r], tau[r], fs) for r in range(ROWS)])
    assert np.max(np.abs(got - want)) <= 1e-11 * scale_of(x)
    got = run_stage(x, [[('correct', a, t)] for a, t in zip(A, tau)], fs)
    want = np.stack([distortion.correct_reflection(x[r], A[r], tau[r], fs) for r in range(ROWS)])
    assert np.max(np.abs(got - want)) <= 1e-11 * scale_of(x)


def test_large_phase():
    """tau = 5 us at 2 GS/s: 10 000 samples of delay, 5 000 cycles of phase at Nyquist.  A delay by a whole number of
    samples is np.roll in exact arithmetic.  The bump is one sample wide (sigma), so the bins up to Nyquist carry
    weight: the reference formula itself is at 7.2e-13 here (NumPy, float64), a phase held in float32 at 7.6e-6."""
    n, fs, tau = 65536, 2e9, 5e-6
    x = np.exp(-0.5 * ((np.arange(n) - 20000) / 1.0)**2)[None, :]
    got = run_stage(x, [[('delay', tau)]], fs)[0]
    err = np.max(np.abs(got - np.roll(x[0], 10000)))
    print(f'large phase: max err {err:.3g}')
    assert err <= 1e-11 * scale_of(x)
    back = run_stage(got[None, :], [[('delay', -tau)]], fs)[0]
    assert np.max(np.abs(back - x[0])) <= 1e-11 * scale_of(x)


def test_strides_in_place_and_streams():
    n, fs = 4099, 2e9
    x, terms = rows_input(n, ROWS, 31), rows_terms(ROWS, 32)
    want = ref_rows(x, terms, fs)
    tol = 1e-11 * scale_of(x)
    st = distortion.ReflectionStage(terms, n, fs)
    wide = torch.full((ROWS, n + 37), 7.0, dtype=torch.float64, device=dev())
    win = wide[:, 5:5 + n]                         # rows start 40 B past an allocation boundary, stride n + 37
    win.copy_(torch.from_numpy(x))
    out = torch.full((ROWS, n + 64), -3.0, dtype=torch.float64, device=dev())
    res = st.apply_torch(win, out=out[:, :n])
    assert res.data_ptr() == out.data_ptr()
    assert np.max(np.abs(out[:, :n].cpu().numpy() - want)) <= tol
    assert bool((out[:, n:] == -3.0).all())                        # nothing written past a row
    assert np.array_equal(win.cpu().numpy(), x)                    # the input is intact
    st.apply_torch(win)                                            # in place, on the window
    assert np.max(np.abs(win.cpu().numpy() - want)) <= tol
    assert bool((wide[:, :5] == 7.0).all()) and bool((wide[:, 5 + n:] == 7.0).all())
    # a contiguous input to a strided output and back to a contiguous one
    xc = torch.from_numpy(x).to(dev())
    assert np.max(np.abs(st.apply_torch(xc, out=out[:, 3:3 + n]).cpu().numpy() - want)) <= tol
    yc = torch.empty_like(xc)
    assert np.max(np.abs(st.apply_torch(win.copy_(xc), out=yc).cpu().numpy() - want)) <= tol
    # a side stream: produced and consumed on it, no synchronisation in between
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z = torch.from_numpy(x).to(dev(), non_blocking=False)
        doubled = st.apply_torch(z) * 2.0
    side.synchronize()
    assert np.max(np.abs(doubled.cpu().numpy() - 2.0 * want)) <= 2 * tol
    # refused shapes
    for bad in (xc[:4], xc[:, :n - 1], xc.to(torch.float32), xc.cpu(), xc.t().contiguous().t()):
        with pytest.raises(ValueError):
            st.apply_torch(bad)
    st.close()


def test_fp32():
    """float32 rows: the bound is measured, not guessed -- the existing SpectralPlan(..., float32) path with a
    host-built H on the same rows, against the float64 formula; the new stage may be 2x that far off.
    (Measured on an MI355X: both paths 2.0e-6 at scale 6.6, i.e. 3e-7 of scale -- float32 transforms of 4096 points;
    the way H is obtained does not show.)"""
    n, fs = 4096, 2e9
    x, terms = rows_input(n, ROWS, 105), rows_terms(ROWS, 205)
    x32 = x.astype(np.float32)
    want = ref_rows(x32.astype(np.float64), terms, fs)
    f = np.fft.rfftfreq(n, 1 / fs)
    base = 0.0
    plan = _engine.SpectralPlan(n, 1, np.float32)
    for r in range(ROWS):
        xin = torch.from_numpy(x32[r]).to(dev())
        y = torch.empty_like(xin)
        H = torch.from_numpy(transfer(terms[r], f)).to(dev())
        plan.apply(xin.data_ptr(), y.data_ptr(), H.data_ptr(), torch.cuda.current_stream().cuda_stream)
        base = max(base, float(np.max(np.abs(y.cpu().numpy() - want[r]))))
    plan.close()
    got = run_stage(x32, terms, fs, np.float32)
    assert got.dtype == np.float32
    err = float(np.max(np.abs(got - want)))
    print(f'fp32: stage max err {err:.3g}, SpectralPlan float32 with host H {base:.3g} (scale {scale_of(x):.3g})')
    assert base > 0 and err <= 2 * base


def test_round_trip():
    """correct after reflect returns the input up to the Nyquist bin of an even-length row, whose imaginary part the
    real transform discards (tests/test_gpu_spectral.py: the reference does the same); not a device error.
    That bin comes back as X_N Re(H) Re(1/H) = X_N (1 - sin^2(arg H)) and |sin(arg H)| <= |A|, so the round trip is off by
    at most A^2 |X_N| / n per sample, X_N = sum (-1)^m x[m]: |A| <= 0.05 keeps that below the 1e-6 of scale asked for
    (it is A^2 that the bound limits: the reference's own round trip is 6e-5 off at |A| = 0.3 on these rows).  A row of
    odd length has no such bin and comes back to rounding; the device's round trip is the reference's to 3e-11 (two
    stages at 1e-11 each, the second one's gain (1 + |A|) / (1 - |A|) on the first one's error)."""
    fs = 1e9
    rng = np.random.default_rng(41)
    A, tau = rng.uniform(-0.05, 0.05, ROWS), rng.uniform(0, 200e-9, ROWS)
    refl, corr = [[('reflect', a, t)] for a, t in zip(A, tau)], [[('correct', a, t)] for a, t in zip(A, tau)]
    for n in (4096, 4097):
        x = rows_input(n, ROWS, 42)
        nyquist = np.abs((x * (-1.0)**np.arange(n)).sum(axis=1))
        assert np.max(A**2 * nyquist / n) <= 1e-6 * scale_of(x)       # (the case is a fair one)
        back = run_stage(run_stage(x, refl, fs), corr, fs)
        print(f'round trip n={n}: {np.max(np.abs(back - x)):.3g}')
        assert np.max(np.abs(back - x)) <= (1e-6 if n % 2 == 0 else 3e-11) * scale_of(x)
        assert np.max(np.abs(back - ref_rows(ref_rows(x, refl, fs), corr, fs))) <= 3e-11 * scale_of(x)


def test_numpy_wrappers():
    n, fs = 1000, 2e9
    x = rows_input(n, 3, 51)
    A, tau = [0.1, [0.2, -0.05], -0.15], [12e-9, [5e-9, 40e-9], 7.5e-9]
    terms = [[('reflect', 0.1, 12e-9)], [('reflect', 0.2, 5e-9), ('reflect', -0.05, 40e-9)], [('reflect', -0.15, 7.5e-9)]]
    tol = 1e-11 * scale_of(x)
    assert np.max(np.abs(distortion.reflection_rows(x, A, tau, fs) - ref_rows(x, terms, fs))) <= tol
    inv = [[('correct',) + t[1:] for t in row] for row in terms]
    assert np.max(np.abs(distortion.correct_reflection_rows(x, A, tau, fs) - ref_rows(x, inv, fs))) <= tol
    shared = distortion.correct_reflection_rows(x, 0.1, 12e-9, fs)          # scalars: every row
    assert np.max(np.abs(shared - ref_rows(x, [[('correct', 0.1, 12e-9)]] * 3, fs))) <= tol
    d = distortion.delay_rows(x, [1.5e-9, -4e-9, 0.0], fs)
    assert np.array_equal(d[2], x[2]) or np.max(np.abs(d[2] - x[2])) <= tol
    assert np.max(np.abs(d[1] - np.roll(x[1], -8))) <= tol                  # -4 ns at 2 GS/s: 8 samples earlier
    assert np.max(np.abs(d - ref_rows(x, [[('delay', 1.5e-9)], [('delay', -4e-9)], [('delay', 0.0)]], fs))) <= tol
    assert distortion.delay_rows(np.zeros((2, 0)), 1e-9, fs).shape == (2, 0)
