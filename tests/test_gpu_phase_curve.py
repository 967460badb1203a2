"""`distortion.phase_curve` / `PhaseCurve` on the device (csrc/wfk_probe.hip behind the per-row IIR launch with one
shared input row) against the host referees of tests/phase_curve_ref.py.

Expected values: one and two time constants -- the reference's arithmetic (`ref.restated`: lfilter on the combined
(b, a), np.convolve, np.interp; bit for bit the reference's function, tests/test_phase_curve_cpu.py), admitted only
where that arithmetic is itself within 1e-10 * scale of the long-double recurrence of the same (b, a) (asserted);
three and four constants -- the np.longdouble cascade (`ref.longdouble_curve`), which the reference only approximates
(5e-10 / 5e-5 of scale at 2 GS/s).  Bound throughout: the project's IIR bound max(1e-9 * scale, 10 * self_err),
scale = max(1, |want|.max()), self_err = the referee's own distance from the long-double curve (0 for the long-double
referee).  Everything said to be bitwise is compared with np.array_equal."""
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy.optimize import curve_fit

import phase_curve_ref as ref
import waveforms_amd as wf
from waveforms_amd import _engine, distortion

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda', 0)
DF = ref.DF_DPHI

P1 = [-0.03, 0.1e-6]
P1P = [0.02, 0.3e-6]
P2 = [-0.03, 0.1e-6, 0.02, 0.3e-6]
P3 = P2 + [0.01, 2e-6]
P4 = P3 + [-0.005, 5e-6]
T_EDGE = np.concatenate([ref.DEMO_T, [-20e-6, 20e-6, 20e-6 - 0.5e-9, 0.0]])      # reaches -lim and +lim
T_WIDE = np.concatenate([ref.DEMO_T[::3], [-25e-6, 25e-6, 21e-6]])               # max|t| > 20 us: a longer signal

# (sample rate, params, pulse_width, start, t): pulse points / start points / K = pp + sp in the comment
CASES = [
    (2e9, P1, 10e-9, 25e-9, T_EDGE),            # 20 / 69 / 89 (odd)   the demo's fit kernel
    (2e9, P2, 10e-9, 25.5e-9, T_EDGE),          # 20 / 70 / 90 (even)
    (2e9, P1P, 0.5e-9, 0.0, ref.DEMO_T),        # 1 / 0 / 1            one sample, no delay
    (1e9, P2, 2e-6, 25e-9, ref.DEMO_T),         # 2000 / 2024 / 4024 (even)
    (2e9, P2, 10e-9, 0.0, T_WIDE),              # 20 / 19 / 39         100000 samples
    (2e9, P1P, 10e-9, 0.0, np.float64(1e-7)),   # a scalar t
    (2e9, P3, 10e-9, 25e-9, T_EDGE),
    (2e9, P4, 2e-6, 0.0, ref.DEMO_T),           # 4000 / 3999 / 7999 (odd)
    (1e9, P4, 10e-9, 25e-9, T_WIDE),
    (1e9, P3, 1e-9, 0.0, np.float64(-1e-6)),    # 1 / 0 / 1, a scalar t inside the pulse
]


def demo_wave():
    return 0.1 * (wf.square(2e-6) << 1e-6)          # reference distortion.py:381


def expected(rate, params, pw, start, t, wav):
    """-> (want, self_err)"""
    args = (t, params, DF, pw, start, wav, rate)
    if len(params) // 2 <= 2:
        want = ref.restated(*args)
        self_err = float(np.max(np.abs(want - ref.combined_longdouble_curve(*args))))
        assert self_err < 1e-10 * ref.scale(want), ('the reference itself is not trustworthy here', self_err)
        return want, self_err
    return ref.longdouble_curve(*args), 0.0


@pytest.mark.parametrize('case', range(len(CASES)))
def test_drop_in_phase_curve(case):
    rate, params, pw, start, t = CASES[case]
    wav = demo_wave()
    got = distortion.phase_curve(t, params, DF, pw, start, wav, rate)
    want, self_err = expected(rate, params, pw, start, t, wav)
    assert type(got) is type(np.interp(t, [0.0, 1.0], [0.0, 1.0])) and np.shape(got) == np.shape(t)
    assert np.asarray(got).dtype == np.float64
    s = ref.scale(want)
    tol = max(1e-9 * s, 10 * self_err)
    err = float(np.max(np.abs(got - want)))
    print(f'case {case}: {len(params) // 2} constants, err {err:.3g}, scale {s:.3g}, self_err {self_err:.3g}, tol {tol:.3g}')
    assert err <= tol, (case, err, tol)


def test_rows_equal_single_calls_bitwise_wherever_they_sit():
    wav = demo_wave()
    pc = distortion.PhaseCurve(T_EDGE, DF, 10e-9, 25e-9, wav, 2e9)
    rows = [P1, P4, P2, [], P3, P1P, P4, P1, P2[2:] + P2[:2], P4]
    got = pc.rows(rows)
    assert got.shape == (len(rows), len(T_EDGE)) and got.dtype == np.float64
    for r, p in enumerate(rows):
        assert np.array_equal(got[r], pc(p)), r
    assert np.array_equal(got[1], got[6]) and np.array_equal(got[1], got[9]) and np.array_equal(got[0], got[7])
    assert np.array_equal(pc.rows(rows[::-1]), got[::-1])
    assert np.array_equal(pc.rows(rows), got)                          # and twice the same
    # no time constant at all: the wave itself through the probe
    x = wav(pc.tlist)
    conv = np.convolve(2 * np.pi * DF * x, np.hstack([np.ones(pc.pp) / 2e9, np.zeros(pc.sp)]), mode='same')
    want = np.interp(T_EDGE, pc.tlist, conv)
    assert np.max(np.abs(got[3] - want)) <= 1e-12 * ref.scale(want)
    # a device tensor of the caller's, written in place; a smaller batch after a larger one (the workspace is kept)
    out = torch.full((3, len(T_EDGE) + 5), 7.0, dtype=torch.float64, device=DEV)
    assert pc.rows_torch(rows[:3], out=out[:, :len(T_EDGE)]).data_ptr() == out.data_ptr()
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :len(T_EDGE)], got[:3]) and np.all(o[:, len(T_EDGE):] == 7.0)
    with pytest.raises(ValueError):
        pc.rows_torch(rows[:3], out=out[:2, :len(T_EDGE)])
    pc.close()


def test_more_than_four_constants_take_the_slow_path_inside_a_batch():
    """Measured on an MI355X with the row sent through `distort()` (the device's order-5 direct form) instead: err 21
    at scale 27 against a bound of 0.015 -- that form does not carry five clustered poles over 40 000 samples, which
    is why further constants run as further cascade passes."""
    wav = demo_wave()
    # (1 GS/s and time constants a factor 3 apart: a combined order-5 direct form that double precision still carries)
    five = [0.01, 20e-9, 0.01, 60e-9, 0.01, 200e-9, 0.01, 700e-9, 0.01, 2.5e-6]
    pc = distortion.PhaseCurve(ref.DEMO_T, DF, 10e-9, 25e-9, wav, 1e9)
    rows = [P2, five, P1]
    got = pc.rows(rows)
    assert np.array_equal(got[0], pc(P2)) and np.array_equal(got[2], pc(P1))
    # the fifth constant is a second in-place IIR launch over the workspace; compared with the reference's arithmetic
    # (the combined order-5 direct form) under that form's own error
    args = (ref.DEMO_T, five, DF, 10e-9, 25e-9, wav, 1e9)
    want = ref.restated(*args)
    self_err = float(np.max(np.abs(want - ref.longdouble_curve(*args))))
    err = float(np.max(np.abs(got[1] - want)))
    print(f'five constants: err {err:.3g}, self_err {self_err:.3g}, scale {ref.scale(want):.3g}')
    assert err <= max(1e-9 * ref.scale(want), 10 * self_err)
    pc.close()


def test_jacobian_is_differences_of_single_calls_bitwise():
    pc = distortion.PhaseCurve(ref.DEMO_T, DF, 10e-9, 25e-9, demo_wave(), 2e9)
    for p, rel in ((np.array(P2), None), (np.array(P3), 1e-6), (np.array([0.0, 0.2e-6]), None)):
        J = pc.jac(p, rel)
        h = pc.step(p, rel)
        assert J.shape == (len(ref.DEMO_T), len(p))
        f0 = pc(p)
        for k in range(len(p)):
            pk = p.copy()
            pk[k] = p[k] + h[k]
            assert np.array_equal(J[:, k], (pc(pk) - f0) / h[k]), k
        assert np.array_equal(pc.jac_model(None, *p), pc.jac(p)) and np.array_equal(pc.model(None, *p), f0)
    pc.close()


def test_shared_input_equals_replicated_input_bitwise_and_overlap_is_refused():
    n, batch = 3 * 4096 + 77, 5
    rng = np.random.default_rng(11)
    secs = [ref.sections(p, 2e9) for p in (P1, P2, P3, P4, P1P)]
    plan = _engine.IirRowsPlan(secs, n, np.float64)
    big = torch.zeros((batch + 2, n), dtype=torch.float64, device=DEV)
    big[batch + 1] = torch.from_numpy(rng.standard_normal(n)).to(DEV)
    x = big[batch + 1]
    a = torch.empty((batch, n), dtype=torch.float64, device=DEV)
    plan.apply_shared_in(x.data_ptr(), a.data_ptr(), n)
    rep = x.repeat(batch, 1).contiguous()
    b = torch.empty_like(rep)
    plan.apply(rep.data_ptr(), n, b.data_ptr(), n)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    # out right in front of in: allowed; out reaching into in, in inside out, out == in: refused, nothing launched
    plan.apply_shared_in(big[batch].data_ptr(), big.data_ptr(), n)
    for in_row, out_row in ((batch - 1, 0), (2, 0), (0, 0)):
        with pytest.raises(_engine.EngineError, match='overlaps'):
            plan.apply_shared_in(big[in_row].data_ptr(), big[out_row].data_ptr(), n)
    with pytest.raises(_engine.EngineError):
        plan.apply_shared_in(x.data_ptr(), a.data_ptr(), n - 1)       # row stride < n
    with pytest.raises(_engine.EngineError):
        plan.apply(x.data_ptr(), 0, a.data_ptr(), n)                  # the ordinary entry keeps its check
    torch.cuda.synchronize()
    plan.close()


def probe_input(pp, c, n=5000):
    """-> (tlist: any ascending grid of n points, t: probe times inside, outside, on its ends and a NaN, gain)"""
    rng = np.random.default_rng(pp + 13 * c + 100)
    tlist = np.cumsum(rng.uniform(0.5, 1.5, n)) - 2500.0
    t = np.concatenate([rng.uniform(tlist[0] - 50, tlist[-1] + 50, 300), tlist[[0, 1, n - 2, n - 1, 2500]],
                        np.nextafter(tlist[[0, n - 1]], 0.0), [np.nan]])
    return rng, tlist, t, 0.37


def probe_numpy(y, n, tlist, t, pp, c, gain):
    """the probe in NumPy for rows y (rows, >= n): the box sum of pp samples ending c past each sample, from a cumulative
    sum of y with zeros on both sides, interpolated at t -> (want (rows, len(t)), the bound of a row's finite results)"""
    rows = y.shape[0]
    pad = np.zeros((rows, 3 * n + 2 * abs(c) + pp))                  # y with zeros on both sides
    off = n + abs(c) + pp
    pad[:, off:off + n] = y[:, :n]
    cs = np.concatenate([np.zeros((rows, 1)), np.cumsum(pad, axis=1)], axis=1)
    i = np.arange(n)
    conv = gain * (cs[:, off + i + c + 1] - cs[:, off + i + c - pp + 1])
    tol = 1e-12 * gain * (pp + 1) * np.abs(y).max() + 1e-13 * np.abs(cs).max()
    return np.stack([np.interp(t, tlist, conv[r]) for r in range(rows)]), tol


@pytest.mark.parametrize('pp,c', [(37, 18), (37, -10), (1, 0), (0, 5), (700, 3000), (2000, 999)])
def test_raw_probe_plan_against_numpy(pp, c):
    n, rows, stride = 5000, 3, 5003
    rng, tlist, t, gain = probe_input(pp, c, n)
    y = rng.standard_normal((rows, stride))
    plan = _engine.BoxProbePlan(tlist, t, pp, c, gain)
    assert plan.kernel_name() == 'boxprobe_wave'
    yd = torch.from_numpy(y).to(DEV)
    out = torch.full((rows, len(t) + 3), 5.0, dtype=torch.float64, device=DEV)
    plan.apply(yd.data_ptr(), rows, stride, out.data_ptr(), len(t) + 3)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:, len(t):] == 5.0)
    got = o[:, :len(t)]
    wants, tol = probe_numpy(y, n, tlist, t, pp, c, gain)
    for r in range(rows):
        want = wants[r]
        assert np.isnan(got[r, -1]) and np.isnan(want[-1])
        assert np.max(np.abs(got[r, :-1] - want[:-1])) <= tol, (r, np.max(np.abs(got[r, :-1] - want[:-1])), tol)
    for bad in (lambda: plan.apply(yd.data_ptr(), rows, n - 1, out.data_ptr(), len(t)),
                lambda: plan.apply(yd.data_ptr(), rows, stride, out.data_ptr(), len(t) - 1),
                lambda: plan.apply(yd.data_ptr(), -1, stride, out.data_ptr(), len(t)),
                lambda: plan.apply(None, rows, stride, out.data_ptr(), len(t)),
                lambda: _engine.BoxProbePlan(tlist, t, n + 1, c, gain),
                lambda: _engine.BoxProbePlan(tlist, t, -1, c, gain),
                lambda: _engine.BoxProbePlan(tlist, t, pp, c, np.inf),
                lambda: _engine.BoxProbePlan(tlist[::-1], t, pp, c, gain),
                lambda: _engine.BoxProbePlan(tlist, t[:0], pp, c, gain)):
        with pytest.raises(_engine.EngineError) as e:
            bad()
        assert len(str(e.value)) > 20
    plan.close()


def test_plain_c_consumer_probes(tmp_path):
    exe = tmp_path / 'probe_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'probe_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'probed on the device, parity ok' in r.stdout, r.stdout


def test_fit_recovers_known_parameters():
    """Noise-free data from the long-double curve of known two-constant parameters, the fit started 20 % off:
    curve_fit(pc.model, ..., jac=pc.jac_model) must land within 10 x the distance at which the same fit driven by the
    host restatement (curve_fit's own differences) lands.  Distance: max_k |popt_k - truth_k| / |truth_k|.
    Measured on an MI355X: device fit 3.66e-11, host fit 0.0784 (curve_fit's own differences of the host model,
    whose rounding noise is of the order of its step, leave it far from the truth)."""
    truth = np.array(P2)
    wav = demo_wave()
    t = ref.DEMO_T
    y = ref.longdouble_curve(t, truth, DF, 10e-9, 25e-9, wav, 2e9)
    p0 = truth * np.array([1.2, 0.8, 0.8, 1.2])
    pc = distortion.PhaseCurve(t, DF, 10e-9, 25e-9, wav, 2e9)
    x_host = wav(pc.tlist)

    def host_model(tt, *p):
        return ref.restated(tt, p, DF, 10e-9, 25e-9, lambda _t: x_host, 2e9)

    pd, _ = curve_fit(pc.model, t, y, p0=p0, jac=pc.jac_model)
    ph, _ = curve_fit(host_model, t, y, p0=p0)
    dd, dh = (float(np.max(np.abs(p - truth) / np.abs(truth))) for p in (pd, ph))
    print(f'fit distances: device {dd:.3g}, host {dh:.3g}')
    assert dd <= 10 * dh, (dd, dh)
    assert dd < 1e-3                                      # and it is a fit at all, not two equally lost ones
    pc.close()
