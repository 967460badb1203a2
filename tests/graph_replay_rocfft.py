"""The rocFFT-backed applies under graph capture and replay, one leg per FRESH process (run by
tests/test_gpu_graph_replay.py::test_rocfft_backed_applies; needs a GPU).

    python tests/graph_replay_rocfft.py all        # every leg of LEGS in a child process of its own, one after another
    python tests/graph_replay_rocfft.py LEG        # one leg, in this process

A capture the runtime refuses may leave a process unfit for the next capture, so no two legs share a process, and after
a leg that did not end well no further leg is started.  Each leg is what tests/test_gpu_graph_replay.py holds for every
other stage: capture once, replay on feeds A, B, A, each replay against the reference of its feed at the bound of the
stage's own test file, bit for bit against an eager twin plan, the third replay bit for bit the first."""
import os
import subprocess
import sys

import numpy as np

LEGS = ('fir_rocfft', 'spectral_rows', 'extract', 'spectral')
LEG_SECONDS = 120


def _hold(make, feeds, check):
    from graph_replay import eager, replay, sentinels_left
    from row_windows import bits_equal
    rig, twin = make(), make()
    got = replay(rig[0], rig[1], feeds, rig[2])
    for k, feed in enumerate(feeds):
        assert all(sentinels_left(o) == 0 for o in got[k]), k
        check(k, got[k])
        tw = eager(twin[0], twin[1], feed, twin[2])
        assert all(bits_equal(a, b) for a, b in zip(got[k], tw)), f'replay {k} differs from the eager twin'
    assert all(bits_equal(a, b) for a, b in zip(got[2], got[0])), 'the third replay differs from the first'
    rig[3]()
    twin[3]()


def leg_fir_rocfft():
    """FirStage under WFK_FIR_ROCFFT=1: the overlap-save pipeline (tests/test_gpu_row_windows.py: FIR_CASES['rocfft'])"""
    import torch
    import test_gpu_row_windows as near
    from cases import FP64_FIR_TOL
    from oracle import c_oracle
    from waveforms_amd import distortion
    K, env = near.FIR_CASES['rocfft']
    rows, n = 4, 20011
    ker = np.random.default_rng(K).normal(size=K)
    ker /= np.abs(ker).sum()
    xs = [np.random.default_rng(s).normal(size=(rows, n)) for s in (K + 1, K + 2)]
    wants = [np.stack([c_oracle.fir(row, ker) for row in x]) for x in xs]

    def make():
        st = distortion.FirStage(ker, n, rows, np.float64)
        x, out = (torch.empty((rows, n), dtype=torch.float64, device='cuda') for _ in range(2))
        return (lambda: st.apply_torch(x, out)), [x], [out], st.close

    def check(k, outs):
        want = wants[k % 2]
        assert np.max(np.abs(outs[0] - want)) <= FP64_FIR_TOL * near._peak(want), k

    with near._env(env):
        _hold(make, [(xs[0], ), (xs[1], ), (xs[0], )], check)


def _reflection_feeds(n, rows):
    import reflection_rows_ref as refl
    fs = 2e9
    terms = refl.rows_terms(5, 32 + n)[2:2 + rows]
    xs = [refl.rows_input(n, rows, s + n) for s in (31, 32)]
    return fs, terms, xs, [refl.ref_rows(x, terms, fs) for x in xs]


def leg_spectral_rows():
    """ReflectionStage (wfk_spectral_rows_apply), in place"""
    import torch
    import test_gpu_reflection_rows as refl_file
    from waveforms_amd import distortion
    n, rows = 4096, 2
    fs, terms, xs, wants = _reflection_feeds(n, rows)

    def make():
        st = distortion.ReflectionStage(terms, n, fs, np.float64)
        x = torch.empty((rows, n), dtype=torch.float64, device='cuda')
        return (lambda: st.apply_torch(x)), [x], [x], st.close

    def check(k, outs):
        assert np.max(np.abs(outs[0] - wants[k % 2])) <= 1e-11 * refl_file.scale_of(xs[k % 2]), k

    _hold(make, [(xs[0], ), (xs[1], ), (xs[0], )], check)


def leg_spectral():
    """SpectralPlan (wfk_spectral_apply): one H for all rows, H fed with the rows"""
    import torch
    import reflection_rows_ref as refl
    from waveforms_amd import _engine
    n, rows, fs = 4096, 2, 2e9
    f = np.fft.rfftfreq(n, 1 / fs)
    terms = refl.rows_terms(5, 32 + n)[2:4]
    Hs = [refl.transfer(t, f) for t in terms]
    xs = [refl.rows_input(n, rows, s + n) for s in (41, 42)]
    wants = [np.stack([refl.ref_row(row, t, fs) for row in x]) for x, t in zip(xs, terms)]

    def make():
        plan = _engine.SpectralPlan(n, rows, np.float64)
        x, out = (torch.empty((rows, n), dtype=torch.float64, device='cuda') for _ in range(2))
        H = torch.empty(n // 2 + 1, dtype=torch.complex128, device='cuda')
        args = (x.data_ptr(), out.data_ptr(), H.data_ptr())
        return (lambda: plan.apply(*args, torch.cuda.current_stream().cuda_stream)), [x, H], [out], plan.close

    def check(k, outs):
        err = np.abs(outs[0] - wants[k % 2]).max(axis=1)
        assert np.all(err <= 1e-11 * np.maximum(1.0, np.abs(xs[k % 2]).max(axis=1))), (k, err)

    _hold(make, [(xs[0], Hs[0]), (xs[1], Hs[1]), (xs[0], Hs[0])], check)


def leg_extract():
    """KernelExtractor (wfk_extract_rows_apply); feed B is feed A with its two rows exchanged: every sample differs and
    the rows are ones the referee's own rule has passed (tests/test_gpu_far_rows.py: EXTRACT_SEEDS)"""
    import torch
    import extract_rows_ref
    import test_gpu_extract_rows as extract_file
    import test_gpu_far_rows as far
    from waveforms_amd import distortion
    n, skip, M, rows = far.EXTRACT_N, far.EXTRACT_SKIP, far.EXTRACT_M, 2
    k = n - 2 * skip
    a, b = extract_file.rows_input(n, rows, far.EXTRACT_SEEDS)
    bw = extract_file.bw_of(M)
    feeds = [(a, b), (a[::-1].copy(), b[::-1].copy())]
    wants = [extract_rows_ref.rows_ref(fa, fb, extract_rows_ref.taps_of(extract_file.FS, bw), skip, (n, M)) for fa, fb in feeds]
    assert np.all(feeds[0][0] != feeds[1][0]) and np.all(feeds[0][1] != feeds[1][1])

    def make():
        ex = distortion.KernelExtractor(n, rows, extract_file.FS, bw, skip)
        ad, bd = (torch.empty((rows, n), dtype=torch.float64, device='cuda') for _ in range(2))
        out = torch.empty((rows, k), dtype=torch.float64, device='cuda')
        return (lambda: ex.apply_torch(ad, bd, out)), [ad, bd], [out], ex.close

    def check(j, outs):
        wants[j % 2].check(outs[0], f'extract replay {j}')

    _hold(make, [feeds[0], feeds[1], feeds[0]], check)


def main(argv):
    here = os.path.dirname(os.path.abspath(__file__))
    if argv[1:] == ['all']:
        for leg in LEGS:
            try:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), leg], timeout=LEG_SECONDS)
            except subprocess.TimeoutExpired:
                print(f'{leg}: ran past {LEG_SECONDS} s; no further leg is started', flush=True)
                return 1
            if res.returncode != 0:
                print(f'{leg}: exit status {res.returncode}; no further leg is started', flush=True)
                return 1
        return 0
    if len(argv) != 2 or argv[1] not in LEGS:
        print(__doc__)
        return 2
    sys.path[:0] = [os.path.dirname(here), here]
    globals()['leg_' + argv[1]]()
    print(f'{argv[1]}: ok', flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
