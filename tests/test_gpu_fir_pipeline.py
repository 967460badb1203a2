"""The rocFFT overlap-save pipeline behind wfk_fir_* (csrc/wfk_fir.hip, fir_run) where tests/test_gpu_fir.py does not
reach: the loop over chunks of rows with its tail plans (WFK_FIR_CHUNK brings it down to test size; unset, it starts
at about 3 GB of staging), transform lengths other than the default (WFK_FIR_L), strided input and padded output rows
and float32 at every one of them, and what the stage refuses: a row of more than 65535 blocks, at creation and before
anything is allocated, and an output that overlaps the input, on every path.

References: oracle.np_oracle.predistort_fir (the reference's fftconvolve restated) and, where n * K < 2e7, the
time-domain sum oracle.c_oracle.fir.  Rows are independent normals, row r times 10**(r % 3), and the fp64 bound is PER
ROW, 1e-12 * max(1, max|want[r]|) (the bound of tests/test_gpu_fir.py): under a bound over all rows a small row that
was swapped with another small one, or left over from the apply before, would hide behind the large ones.  float32:
sum|ker| = 1 and unit-normal rows, 1e-5 absolute, as in tests/test_gpu_fir.py.

Every apply reads rows `n + 5` apart (the gaps hold 1e30: a window that strays past its row shows) and writes rows
`n + 13` apart into a buffer of 7.0, whose padding must come back bit-identical.  Every plan is applied twice, to
different data: the staging buffers `win` and `spec` are reused from chunk to chunk and from apply to apply."""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu
IN_PAD, OUT_PAD = 5, 13


def dev():
    return torch.device('cuda', torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def problem(K, n, batch):
    """-> [(ker64, x64, wants64), (ker32, x32, wants32)]; x and every array of `wants` (np_oracle's and, where
    n * K < 2e7, c_oracle's) have shape (2, batch, n): the data of the two applies.  Computed once per shape and
    shared, read-only, by the tests that use it."""
    rng = np.random.default_rng(1000003 * K + 101 * n + batch)
    ker = rng.normal(size=K)
    unit = ker / np.abs(ker).sum()
    x = rng.normal(size=(2, batch, n))
    scaled = x * (10.0 ** (np.arange(batch) % 3))[None, :, None]
    out = []
    for k, sig in ((ker, scaled), (unit, x)):
        wants = [np.stack([[np_oracle.predistort_fir(row, k) for row in app] for app in sig])]
        if n * K < 2e7:
            wants.append(np.stack([[c_oracle.fir(row, k) for row in app] for app in sig]))
        for a in [k, sig] + wants:
            a.setflags(write=False)
        out.append((k, sig, wants))
    return out


def check_plan(K, n, batch, label):
    """fp64 and fp32 plans of the shape under the environment the caller has set: two applies each, strided in,
    padded out"""
    for (ker, x, wants), dt, tdt in zip(problem(K, n, batch), (np.float64, np.float32), (torch.float64, torch.float32)):
        st = distortion.FirStage(ker, n, batch, dt)
        try:
            for a in range(2):
                xd = torch.full((batch, n + IN_PAD), 1e30, dtype=tdt, device=dev())
                xd[:, :n] = torch.from_numpy(x[a]).to(dev(), tdt)
                yd = torch.full((batch, n + OUT_PAD), 7.0, dtype=tdt, device=dev())
                st.apply_torch(xd, yd)
                torch.cuda.synchronize()
                got = yd.cpu().numpy()
                assert got.dtype == dt
                assert np.all(got[:, n:] == dt(7.0)), (label, dt.__name__, a, 'padding written')
                for want in wants:
                    err = np.abs(got[:, :n].astype(np.float64) - want[a]).max(axis=1)
                    if dt == np.float64:
                        tol = 1e-12 * np.maximum(1.0, np.abs(want[a]).max(axis=1))
                    else:
                        tol = np.full(batch, 1e-5)
                    print(f'{label} {dt.__name__} apply {a}: max err / bound per row '
                          + ' '.join(f'{e:.2g}/{t:.2g}' for e, t in zip(err, tol)))
                    assert np.all(err <= tol), (label, dt.__name__, a, err, tol)
        finally:
            st.close()


# ---- the chunk loop ---------------------------------------------------------------------------------------------
# K = 33 at L = 1024: hop M = 992, n = 9000 is 10 blocks per row (the last one 72 samples)
CHUNKS = [(5, 2),    # two full chunks and a tail of one row
          (4, 2),    # no tail
          (3, 5),    # the knob above the batch: one chunk
          (7, 3),
          (1, 1),
          (5, 1)]    # every chunk a single row


@pytest.mark.parametrize('batch,chunk', CHUNKS)
def test_chunked_rows(batch, chunk, monkeypatch):
    monkeypatch.setenv('WFK_FIR_ROCFFT', '1')
    monkeypatch.setenv('WFK_FIR_L', '1024')
    monkeypatch.setenv('WFK_FIR_CHUNK', str(chunk))
    check_plan(33, 9000, batch, f'chunk {chunk} of {batch}')
    # the same rows in one chunk meet the same bound (not compared bit by bit with the chunked result: rocFFT may
    # pick another kernel for another batch count)
    monkeypatch.delenv('WFK_FIR_CHUNK')
    check_plan(33, 9000, batch, f'unchunked {batch}')


def test_chunked_rows_long_kernel(monkeypatch):
    """K = 7000 is past the four segments of the on-chip transform: the pipeline by kernel length, as users reach
    it, at its default transform length (65536; n = 9000 is one block)"""
    monkeypatch.delenv('WFK_FIR_ROCFFT', raising=False)
    monkeypatch.delenv('WFK_FIR_L', raising=False)
    monkeypatch.setenv('WFK_FIR_CHUNK', '2')
    check_plan(7000, 9000, 5, 'K=7000 chunk 2 of 5')
    monkeypatch.delenv('WFK_FIR_CHUNK')
    check_plan(7000, 9000, 5, 'K=7000 unchunked')


@pytest.mark.parametrize('knob', ['0', '-2', '2x', '', 'two', '1.5'])
def test_chunk_knob_ignores_what_is_no_positive_integer(knob, monkeypatch):
    monkeypatch.setenv('WFK_FIR_ROCFFT', '1')
    monkeypatch.setenv('WFK_FIR_L', '1024')
    monkeypatch.setenv('WFK_FIR_CHUNK', knob)
    check_plan(33, 9000, 3, f'WFK_FIR_CHUNK={knob!r}')


def test_more_rows_than_a_launch_takes(monkeypatch):
    """batch > 65535 is the pipeline's by row count, and a chunk's row is the launch's third grid index: the chunk is
    capped at 65535 rows, here 65535 + a tail of 4.  Rows of 40 samples, 5 taps, transform length 16 (hop 12, 4
    blocks): about 70 MB of staging.  The reference is the time-domain sum over all rows at once (exact to a few
    ulp: 5 terms), np_oracle on the rows around the seam."""
    K, n, batch = 5, 40, 65539
    rng = np.random.default_rng(65539)
    ker = rng.normal(size=K)
    x = rng.normal(size=(batch, n)) * (10.0 ** (np.arange(batch) % 3))[:, None]
    padded = np.zeros((batch, n + 2 * K))
    padded[:, K:K + n] = x
    want = np.zeros_like(x)
    for k in range(K):                         # out[i] = sum_k ker[k] x[i + K//2 - k]
        want += ker[k] * padded[:, K + K // 2 - k:K + K // 2 - k + n]
    for r in (0, 65534, 65535, 65538):
        ref = np_oracle.predistort_fir(x[r], ker)
        assert np.max(np.abs(want[r] - ref)) <= 1e-13 * max(1.0, np.abs(ref).max())
    monkeypatch.setenv('WFK_FIR_L', '16')
    monkeypatch.delenv('WFK_FIR_ROCFFT', raising=False)
    monkeypatch.delenv('WFK_FIR_CHUNK', raising=False)
    st = distortion.FirStage(ker, n, batch, np.float64)
    try:
        xd = torch.from_numpy(x).to(dev())
        yd = torch.full((batch, n + OUT_PAD), 7.0, dtype=torch.float64, device=dev())
        st.apply_torch(xd, yd)
        torch.cuda.synchronize()
        got = yd.cpu().numpy()
    finally:
        st.close()
    assert np.all(got[:, n:] == 7.0)
    err = np.abs(got[:, :n] - want).max(axis=1)
    tol = 1e-12 * np.maximum(1.0, np.abs(want).max(axis=1))
    worst = int(np.argmax(err / tol))
    print(f'{batch} rows: worst row {worst}, err {err[worst]:.3g}, bound {tol[worst]:.3g}')
    assert np.all(err <= tol)


# ---- transform lengths ------------------------------------------------------------------------------------------
# K = 100: L = 256 is the smallest legal transform, 2^ceil(log2(2 K)), hop 157; n = 157 is exactly one hop, 1000 and
# 5000 end in a block that starts beyond n - M.  128 (< 2 K) and 300 (no power of two) are ignored: default length.
LENGTHS_N = (1, 99, 157, 1000, 5000)


@pytest.mark.parametrize('L', ['256', '1024', '4096', '128', '300'])
def test_transform_lengths(L, monkeypatch):
    monkeypatch.setenv('WFK_FIR_ROCFFT', '1')
    monkeypatch.setenv('WFK_FIR_L', L)
    for n in LENGTHS_N:
        check_plan(100, n, 2, f'L={L} K=100 n={n}')


@pytest.mark.parametrize('K', [1, 2, 101, 511, 512, 513])
def test_kernel_lengths_at_1024(K, monkeypatch):
    """K = 1, even and odd K at L = 1024.  K = 512 is the smallest legal hop there, L = 2 K (the default would be
    4096); for K = 513 the value is below 2 K and ignored."""
    monkeypatch.setenv('WFK_FIR_ROCFFT', '1')
    monkeypatch.setenv('WFK_FIR_L', '1024')
    for n in LENGTHS_N:
        check_plan(K, n, 2, f'L=1024 K={K} n={n}')


# ---- refusals ---------------------------------------------------------------------------------------------------
def test_too_many_blocks_is_refused_at_creation_without_allocating(monkeypatch):
    """n = 992 * 65536 at hop 992 is 65536 blocks.  The plan could never run (wfk_fir_apply refuses it), and its
    staging would be 1 GB: creation fails, and the device's free memory is what it was."""
    monkeypatch.setenv('WFK_FIR_ROCFFT', '1')
    monkeypatch.setenv('WFK_FIR_L', '1024')
    ker = np.ones(33) / 33
    distortion.FirStage(ker, 9000, 1).close()                # (rocFFT is set up now, whatever that allocates)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises((ValueError, _engine.EngineError), match='blocks > 65535'):
        distortion.FirStage(ker, 992 * 65536, 1)
    with pytest.raises((ValueError, _engine.EngineError), match='blocks > 65535'):
        distortion.FirStage(ker, 992 * 65536, 3, np.float32)
    free1 = torch.cuda.mem_get_info()[0]
    print(f'free memory before {free0}, after {free1}')
    assert abs(free0 - free1) <= 64 << 20
    # the on-chip transform takes the same length: the limit is the pipeline's alone
    monkeypatch.delenv('WFK_FIR_ROCFFT')
    distortion.FirStage(ker, 992 * 65536, 1).close()


PATHS = {'fused': (33, None), 'segments': (2401, None), 'rocfft': (33, '1')}


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_overlapping_out_is_refused(path, dtype, monkeypatch):
    """The identical range, the range one row on, the range 8 bytes on, either way round: WFK_EINVAL from the C ABI
    (EngineError) and ValueError from apply_torch, nothing launched.  Ranges that only touch are accepted."""
    K, force = PATHS[path]
    if force:
        monkeypatch.setenv('WFK_FIR_ROCFFT', force)
    else:
        monkeypatch.delenv('WFK_FIR_ROCFFT', raising=False)
    n, batch = 1000, 3
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    es = np.dtype(dtype).itemsize
    ker, x, wants = problem(K, n, batch)[1]
    st = distortion.FirStage(ker, n, batch, dtype)
    try:
        flat = torch.zeros(2 * (batch + 1) * n, dtype=tdt, device=dev())
        flat[:batch * n] = torch.from_numpy(x[0].reshape(-1)).to(dev(), tdt)
        before = flat.clone()
        base = flat.data_ptr()
        for shift in (0, n * es, 8, batch * n * es - es):          # bytes from in to out; the last: one element shared
            for a, b in ((base, base + shift), (base + shift, base)):
                with pytest.raises(_engine.EngineError, match='wfk error -1'):
                    st.apply(a, n, b, n, torch.cuda.current_stream().cuda_stream)
        rows = flat[:(batch + 1) * n].view(batch + 1, n)
        off = 8 // es
        pairs = [(rows[:batch], rows[:batch]), (rows[:batch], rows[1:]), (rows[1:], rows[:batch]),
                 (flat[:batch * n].view(batch, n), flat[off:off + batch * n].view(batch, n)),
                 (flat[off:off + batch * n].view(batch, n), flat[:batch * n].view(batch, n))]
        for xin, yout in pairs:
            with pytest.raises(ValueError):
                st.apply_torch(xin, yout)
        # strided rows: the ranges run to the END of the last row, not to batch * stride
        wide = flat.view(2, (batch + 1) * n)[0][:batch * (n + 7)].view(batch, n + 7)
        with pytest.raises(ValueError):
            st.apply_torch(wide, flat[(batch - 1) * (n + 7) + n - 1:][:batch * n].view(batch, n))
        torch.cuda.synchronize()
        assert torch.equal(flat, before)                           # a refusal launches nothing
        # out begins where in ends: accepted, and right
        y = flat[batch * n:2 * batch * n].view(batch, n)
        st.apply_torch(flat[:batch * n].view(batch, n), y)
        torch.cuda.synchronize()
        err = np.abs(y.cpu().numpy().astype(np.float64) - wants[0][0]).max()
        assert err <= (1e-12 if dtype == np.float64 else 1e-5)
        assert torch.equal(flat[:batch * n], before[:batch * n])
    finally:
        st.close()


ROW_STAGES = {
    'fir': (lambda n, batch, dt: distortion.FirStage(np.arange(1.0, 10.0) / 45.0, n, batch, dt), False),
    'iir_rows': (lambda n, batch, dt: distortion.IirStage(
        [[distortion.exp_decay_filter(0.02 * (r + 1), (30 + 10 * r) * 1e-9, 2e9)] for r in range(batch)], n, batch, dt),
        True),
    'reflection': (lambda n, batch, dt: distortion.ReflectionStage(
        [[('correct', 0.1 * (r + 1), (3 + r) * 1e-9), ('delay', 0.7e-9 * r)] for r in range(batch)], n, 2e9, dt), True),
    'shift': (lambda n, batch, dt: distortion.ShiftStage([0.3e-9 * (r + 1) for r in range(batch)], n, 0.5e-9, dt),
              False),
}


@pytest.mark.parametrize('name', list(ROW_STAGES))
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_row_rule_is_one_rule_for_every_stage(name, dtype):
    """The shared row check (csrc/wfk_host.h, waveforms_amd/_rows.py) as every per-row stage applies it: a row stride of
    n - 1 and a null buffer are refused (ValueError from apply_torch, WFK_EINVAL from the raw apply), the out-of-place
    stages refuse the overlap cases of test_overlapping_out_is_refused with `overlaps` in the text, the in-place stages
    take out is x; no refusal launches anything, and the stage then computes what a fresh one computes, bit for bit."""
    make, in_place = ROW_STAGES[name]
    n, batch = 70, 3
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    es = np.dtype(dtype).itemsize
    st, fresh = make(n, batch, dtype), None
    try:
        rng = np.random.default_rng(70)
        flat = torch.zeros(2 * (batch + 1) * n, dtype=tdt, device=dev())
        flat[:batch * n] = torch.from_numpy(rng.normal(size=batch * n)).to(dev(), tdt)
        before = flat.clone()
        base = flat.data_ptr()
        x = flat[:batch * n].view(batch, n)
        y = flat[(batch + 1) * n:][:batch * n].view(batch, n)
        raw = st.plan.apply

        def refused_raw(*args, match='wfk error -1'):
            with pytest.raises(_engine.EngineError, match=match) as e:
                raw(*args)
            assert 'wfk error -1' in str(e.value)

        # a row stride below n, on either side
        short = flat.as_strided((batch, n), (n - 1, 1))
        for xin, yout in ((short, y), (x, y.as_strided((batch, n), (n - 1, 1)))):
            with pytest.raises(ValueError):
                st.apply_torch(xin, yout)
        refused_raw(x.data_ptr(), n - 1, y.data_ptr(), n)
        refused_raw(x.data_ptr(), n, y.data_ptr(), n - 1)
        # a null buffer
        refused_raw(x.data_ptr(), n, None, n)
        refused_raw(None, n, y.data_ptr(), n)
        if not in_place:
            for shift in (0, n * es, 8, batch * n * es - es):      # bytes from in to out; the last: one element shared
                for a, b in ((base, base + shift), (base + shift, base)):
                    refused_raw(a, n, b, n, match='overlaps')
            rows = flat[:(batch + 1) * n].view(batch + 1, n)
            off = 8 // es
            wide = flat.view(2, (batch + 1) * n)[0][:batch * (n + 7)].view(batch, n + 7)
            pairs = [(rows[:batch], rows[:batch]), (rows[:batch], rows[1:]), (rows[1:], rows[:batch]),
                     (x, flat[off:off + batch * n].view(batch, n)), (flat[off:off + batch * n].view(batch, n), x),
                     # strided rows: the ranges run to the END of the last row, not to batch * stride
                     (wide, flat[(batch - 1) * (n + 7) + n - 1:][:batch * n].view(batch, n))]
            for xin, yout in pairs:
                with pytest.raises(ValueError, match='overlaps'):
                    st.apply_torch(xin, yout)
        torch.cuda.synchronize()
        assert torch.equal(flat, before)                           # a refusal launches nothing
        # a valid call afterwards: what a fresh stage gives
        fresh = make(n, batch, dtype)
        want = fresh.apply_torch(x, torch.zeros_like(x))
        assert st.apply_torch(x, y) is y
        torch.cuda.synchronize()
        assert torch.equal(y, want) and bool(torch.isfinite(y).all()) and not torch.equal(y, before[:batch * n].view(batch, n))
        assert torch.equal(flat[:batch * n], before[:batch * n])
        if in_place:
            z = x.clone()
            assert st.apply_torch(z, z) is z and st.apply_torch(x.clone()) is not None
            torch.cuda.synchronize()
            assert torch.equal(z, want)
    finally:
        st.close()
        if fresh is not None:
            fresh.close()
