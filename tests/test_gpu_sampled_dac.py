"""The sampler that writes DAC codes itself (distortion.SampledDac: wfk_sample_short_dac in csrc/wfk_short.hip, the plan
in csrc/wfk_chain_dac.hip) against the two launches it replaces -- BatchSampler.launch_torch (float64) followed by
DacStage.apply_torch -- bit for bit, codes and counts: the fused build evaluates the same statements, so every
comparison with the two launches is exact.  One independent referee: tests/dac_rows_ref.py on the reference's own
vectors (tests/golden/awg.npz), exact outside the tie zone that tests/test_sampled_dac_cpu.py holds thin."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import cases
import dac_rows_ref as ref
import golden_io
import waveforms_amd as wf
from test_sampled_dac_cpu import REAL_CASES, referee_parameters, tie_zone
from waveforms_amd import distortion, workloads as wl
from waveforms_amd._sampling import BatchSampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AWG = golden_io.npz('awg.npz')
SENTINEL = -21846                                                                # 0xAAAA
FORMATS = [(16, 0), (14, 2), (2, 14)]                                            # (bits, shift)


def dev():
    return torch.device('cuda', torch.cuda.current_device())


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}')


def two_launches(chans, grid, gain, offset=0.0, bits=16, shift=0, k=1, tile=1):
    """-> (codes, counts, the float64 rows, is the sampler's plan a pure wfk_sample_short launch)"""
    bs = BatchSampler(chans, grid, tile=tile)
    z = torch.empty((bs.n_channels, max(bs.n, 1)), dtype=torch.float64, device=dev())[:, :bs.n]
    if bs.n:
        bs.launch_torch(z)
    name = bs.plan.kernel_name(np.float64)
    st = distortion.DacStage(gain, bs.n, offset=offset, bits=bits, shift=shift, interleave=k, batch=bs.n_channels)
    counts = torch.full((bs.n_channels, 3), 0x5a5a5a5a5a, dtype=torch.int64, device=dev())
    codes = st.apply_torch(z, counts=counts)
    out = codes.cpu().numpy(), counts.cpu().numpy(), z.cpu().numpy(), name.startswith('wfk_sample_short<') and ' + ' not in name
    st.close()
    bs.close()
    return out


def one_launch(sd, counts=True):
    """-> (codes, counts or None) of a launch into fresh tensors, the counts full of garbage before it"""
    y = torch.full((sd.out_rows, sd.out_n), SENTINEL, dtype=torch.int16, device=dev())
    c = torch.full((sd.n_channels, 3), 0x5a5a5a5a5a, dtype=torch.int64, device=dev()) if counts else None
    res = sd.launch_torch(y, c)
    assert res.dtype == torch.int16 and tuple(res.shape) == (sd.out_rows, sd.out_n)
    return res.cpu().numpy(), (c.cpu().numpy() if counts else None)


def check(chans, grid, gain, offset=0.0, bits=16, shift=0, k=1, tile=1, fam=None, what=''):
    """SampledDac == the two launches, with and without counts; fused exactly where the sampler's plan is pure short"""
    want, want_counts, z, pure = two_launches(chans, grid, gain, offset, bits, shift, k, tile)
    sd = distortion.SampledDac(chans, grid, gain, offset, bits, shift, k, tile=tile)
    try:
        assert sd.fused == (pure and k == 1 and sd.n > 0), (what, sd.why_not)
        assert bool(sd.why_not) != sd.fused
        if sd.fused:
            assert sd.kernel_name().startswith('wfk_sample_short_dac<16,') and sd.kernel_name().endswith(',false>')
            assert sd.kernel_name(counts=True).endswith(',true>')
            if fam is not None:
                assert int(sd.kernel_name().split(',')[1]) in fam, (what, sd.kernel_name())
        else:
            assert sd.kernel_name(counts=True).endswith(' + dac_rows_count<double>'), sd.kernel_name(True)
        codes, counts = one_launch(sd)
        same(codes, want, f'{what} codes')
        same(counts, want_counts, f'{what} counts')
        plain, _ = one_launch(sd, counts=False)
        same(plain, want, f'{what} codes of the plain build')
    finally:
        sd.close()
    return want, want_counts, z


@functools.lru_cache(maxsize=None)
def golden_case(name):
    build, rate, n = cases.AWG_CASES[name]
    return build(wf, rate), cases._awg_grid(n, rate), AWG[name + '.y']


@pytest.mark.parametrize('bits,shift', FORMATS)
@pytest.mark.parametrize('name', REAL_CASES)
def test_golden_cases_equal_the_two_launches(name, bits, shift):
    w, grid, y = golden_case(name)
    gain, offset = referee_parameters(y, bits)
    _, want_counts, _ = check([w], grid, gain, offset, bits, shift, what=f'{name} {bits}/{shift}')
    assert want_counts[0, 0] > 0 or want_counts[0, 1] > 0                 # rows clip: the counts are not all zero


@pytest.mark.parametrize('name', ['b2b_2g', 'clip_2g'])
def test_independent_referee_on_the_golden_vectors(name):
    """dac_ref of the REFERENCE's samples: codes equal outside the tie zone and within 1 LSB inside it; counts equal up
    to the zone's samples at the rails"""
    w, grid, y = golden_case(name)
    gain, offset = referee_parameters(y, 14)
    zone, delta = tie_zone(y, gain, offset)
    want, want_counts = ref.dac_ref(y[None], gain, offset, 14, 0)
    sd = distortion.SampledDac([w], grid, gain, offset, bits=14)
    assert sd.fused, sd.why_not
    codes, counts = one_launch(sd)
    sd.close()
    diff = np.abs(codes[0].astype(np.int64) - want[0])
    print(f'{name}: {int(zone.sum())} zone samples (delta {delta:.3g} LSB), {int((diff != 0).sum())} codes differ')
    assert not diff[~zone].any() and diff.max(initial=0) <= 1
    v = y * gain + offset
    lo, hi = ref.rails(14)
    at_rail = int((zone & ((np.abs(v - (hi + 0.5)) <= 2 * delta) | (np.abs(v - (lo - 0.5)) <= 2 * delta))).sum())
    assert counts[0, 2] == 0 and np.all(np.abs(counts[0, :2] - want_counts[0, :2]) <= at_rail)


def pulse_train(t0, n, rate=2e9, seed=3):
    rng = np.random.default_rng(seed)
    w = wf.zero()
    for k in range(n // 60 - 1):
        I, Q = wf.mixing(wf.gaussian(20e-9), freq=rng.uniform(-3e8, 3e8), phase=rng.uniform(0, 6), DRAGScaling=1e-10)
        w = w + ((rng.uniform(0.2, 1) * (I if k % 2 else Q)) >> (t0 + (k + 0.5) * 30e-9))
    return w


FAMILIES = [('flat_top', (1, 2)), ('linear_chirp', (1,)), ('ten_tones', (1,)), ('exp_chirp', (4,)), ('interp', (2,)),
            ('far', (6,))]


@pytest.mark.parametrize('shape,fam', FAMILIES)
def test_every_op_family(shape, fam):
    n, rate = 20000, 2e9
    grid = wl.awg_grid(n, rate)
    if shape == 'interp':
        chans = [wl.awg_interp_channel(wf, c, n, rate) for c in range(4)]
    elif shape == 'far':
        chans = [pulse_train(1e-3, n, rate, seed=c) for c in range(4)]
        grid = ('arange', 1e-3, 1e-3 + n / rate, 1 / rate)
    else:
        chans = [wl.awg_shape_channel(wf, shape, c, n, rate) for c in range(4)]
    gains = [9000.0, -12000.5, 30000.0, 45000.0]
    want, want_counts, _ = check(chans, grid, gains, [0.0, 12.5, -300.25, 0.5], 14, 2, fam=fam, what=shape)
    sd = distortion.SampledDac(chans, grid, gains, bits=14, shift=2)
    assert sd.fused, (shape, sd.why_not)
    sd.close()


def short_pulses(n_rows=2, length=1.2e-5):
    """rows of 60-sample pulses at 2 GS/s, long enough for every grid length used here"""
    return [wl.awg_channel(wf, c, int(length * 2e9), 2e9) for c in range(n_rows)]


@pytest.mark.parametrize('n', [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1007, 1008, 1009, 1023, 1024, 1025, 10007])
def test_grid_lengths(n):
    check(short_pulses(), ('arange', 0.0, n / 2e9, 1 / 2e9), [40000.0, -25000.0], [3.25, -0.5], what=f'n={n}')


@pytest.mark.parametrize('n', [5, 1009, 4099])
def test_row_leads_and_sentinels(n):
    """every lead 0 .. 7 of an output row inside a wider int16 buffer whose row stride is odd: rows start at every
    2-byte offset of a 16-byte group, and nothing around a row is touched"""
    chans = short_pulses(3)
    grid = ('arange', 0.0, n / 2e9, 1 / 2e9)
    gains, offs = [40000.0, -25000.0, 33000.0], [3.25, -0.5, 100.0]
    want, want_counts, _, _ = two_launches(chans, grid, gains, offs, 14, 2)
    sd = distortion.SampledDac(chans, grid, gains, offs, bits=14, shift=2)
    assert sd.fused, sd.why_not
    stride = n + 64 + (n % 2 == 0)
    assert stride % 2 == 1
    for lead in range(8):
        wide = torch.full((3, stride), SENTINEL, dtype=torch.int16, device=dev())
        counts = torch.full((3, 3), -77, dtype=torch.int64, device=dev())
        res = sd.launch_torch(wide[:, lead:lead + n], counts)
        assert res.data_ptr() == wide[:, lead:].data_ptr()
        full = wide.cpu().numpy()
        same(full[:, lead:lead + n], want, f'n={n} lead={lead}')
        assert np.all(full[:, :lead] == SENTINEL) and np.all(full[:, lead + n:] == SENTINEL), (n, lead)
        same(counts.cpu().numpy(), want_counts, f'counts n={n} lead={lead}')
    sd.close()


@pytest.mark.parametrize('name', ['duty30_2g', 'vstack_2g', 'clipping_constant'])
def test_pure_fill_units(name):
    """long stretches of the channel's constant: the code of the constant (vstack_2g: 0.125), and where that code
    clips the stretch is counted sample by sample"""
    if name == 'clipping_constant':
        a = wl.awg_channel(wf, 3, 4000, 2e9)
        w, grid = wf.WaveVStack([a, a >> 20e-6]) + 0.75, ('arange', 0.0, 30e-6, 1 / 2e9)   # 0.75: the channel's offset
        gain, offset = [50000.0], [100.0]                                  # 0.75 * 50000 + 100: above the top rail
    else:
        w, grid, y = golden_case(name)
        gain, offset = [1.1 * 32767 / float(np.abs(y).max())], [-250.5]
    want, want_counts, z = check([w], grid, gain, offset, what=name)
    if name == 'clipping_constant':
        assert want_counts[0, 1] > 40000 and np.count_nonzero(z[0] == 0.75) > 40000


def test_counts_are_overwritten_and_refused_where_they_overlap():
    chans, grid = short_pulses(4), wl.awg_grid(5000, 2e9)
    want, want_counts, _, _ = two_launches(chans, grid, 50000.0, 0.5)
    assert want_counts[:, :2].min() > 0
    sd = distortion.SampledDac(chans, grid, 50000.0, 0.5)
    y = torch.empty((4, 5000), dtype=torch.int16, device=dev())
    c = torch.full((4, 3), -12345, dtype=torch.int64, device=dev())
    sd.launch_torch(y, c)
    same(c.cpu().numpy(), want_counts, 'counts out of garbage')
    sd.launch_torch(y, c)
    same(c.cpu().numpy(), want_counts, 'counts of a second launch')
    same(y.cpu().numpy(), want, 'codes')
    over = y.view(-1)[16:16 + 48].view(torch.int64).view(4, 3)
    with pytest.raises(ValueError, match='overlaps'):
        sd.launch_torch(y, over)
    from waveforms_amd import _engine
    with pytest.raises(_engine.EngineError, match='counts overlaps out'):
        sd.launch(y.data_ptr(), 5000, y.data_ptr() + 64)
    with pytest.raises(_engine.EngineError, match='not aligned to their element'):
        sd.launch(y.data_ptr() + 1, 5000)
    with pytest.raises(_engine.EngineError, match='out row stride smaller'):
        sd.launch(y.data_ptr(), 4999)
    for bad in (c[:3], c.to(torch.int32), c.cpu()):
        with pytest.raises(ValueError, match='counts'):
            sd.launch_torch(y, bad)
    for bad in (y[:3], y[:, :4999], y.to(torch.int32), y.cpu()):
        with pytest.raises(ValueError, match='codes'):
            sd.launch_torch(bad)
    sd.close()


def test_reproducible_and_independent_of_the_batch():
    n = 10007
    grid = ('arange', 0.0, n / 2e9, 1 / 2e9)
    row = wl.awg_channel(wf, 5, n, 2e9, True)
    others = [wl.awg_channel(wf, c, n, 2e9) for c in range(3)]
    g0, o0 = 41000.5, -17.25

    def run(chans, gains, offs, tile=1):
        sd = distortion.SampledDac(chans, grid, gains, offs, tile=tile)
        assert sd.fused
        a, ca = one_launch(sd)
        b, cb = one_launch(sd)
        sd.close()
        assert np.array_equal(a, b) and np.array_equal(ca, cb)
        return a, ca
    alone, c_alone = run([row], [g0], [o0])
    assert c_alone[0, :2].min() > 0
    first, c_first = run([row] + others * 21, [g0] + [30000.0] * 63, [o0] + [1.5] * 63)
    last, c_last = run(others * 21 + [row], [30000.0] * 63 + [g0], [1.5] * 63 + [o0])
    assert first.shape[0] == 64
    assert np.array_equal(first[0], alone[0]) and np.array_equal(c_first[0], c_alone[0])
    assert np.array_equal(last[63], alone[0]) and np.array_equal(c_last[63], c_alone[0])


def test_unfused_paths(monkeypatch):
    chans, grid = short_pulses(4), wl.awg_grid(4099, 2e9)
    gains, offs = [40000.0, -25000.0, 33000.0, 50000.0], [3.25, -0.5, 100.0, 0.0]
    check(chans, grid, gains, offs, k=2, what='interleave 2')
    sd = distortion.SampledDac(chans, grid, gains, offs, interleave=2)
    assert not sd.fused and 'interleave' in sd.why_not and sd.kernel_name().endswith(' + dac_rows<double>')
    sd.close()
    want, want_counts, _, pure = two_launches(chans, grid, gains, offs)
    monkeypatch.setenv('WFK_CHAIN_UNFUSED', '1')
    sd = distortion.SampledDac(chans, grid, gains, offs)
    monkeypatch.delenv('WFK_CHAIN_UNFUSED')
    assert pure and not sd.fused and 'WFK_CHAIN_UNFUSED' in sd.why_not
    codes, counts = one_launch(sd)
    same(codes, want, 'WFK_CHAIN_UNFUSED codes')
    same(counts, want_counts, 'WFK_CHAIN_UNFUSED counts')
    from waveforms_amd import _engine
    with pytest.raises(_engine.EngineError, match='needs scratch'):
        sd.plan.launch(torch.empty((4, 4099), dtype=torch.int16, device=dev()).data_ptr(), 4099)
    sd.close()
    # long pieces: the sampler's plan is not a short plan
    long_chans = [wl.sum_channel(wf, 6, 1000 + c) for c in range(2)]
    check(long_chans, ('linspace', 0.0, 6 * wl.SPAN, 12001, False), [30000.0, 50000.0], what='long pieces')


def test_empty_grid_side_stream_and_graph_replay():
    chans = short_pulses(2)
    sd = distortion.SampledDac(chans, ('arange', 0.0, 0.0, 1 / 2e9), 1000.0)
    assert sd.n == 0 and not sd.fused and sd.why_not
    assert tuple(sd.launch_torch(torch.empty((2, 0), dtype=torch.int16, device=dev())).shape) == (2, 0)
    codes, counts = sd.to_host(return_counts=True)
    assert codes.shape == (2, 0) and not counts.any()
    sd.close()
    grid = wl.awg_grid(4099, 2e9)
    want, want_counts, _, _ = two_launches(chans, grid, [40000.0, -52000.0], 0.5)
    sd = distortion.SampledDac(chans, grid, [40000.0, -52000.0], 0.5)
    assert sd.fused
    host, host_counts = sd.to_host(return_counts=True)
    same(host, want, 'to_host codes')
    same(host_counts, want_counts, 'to_host counts')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = torch.full((2, 4099), SENTINEL, dtype=torch.int16, device=dev())
        c = torch.full((2, 3), 99, dtype=torch.int64, device=dev())
        y2, c2 = sd.launch_torch(y, c) + 0, c + 0
    side.synchronize()
    same(y2.cpu().numpy(), want, 'side stream codes')
    same(c2.cpu().numpy(), want_counts, 'side stream counts')
    # one capture and one replay of a fused launch with counts
    y = torch.full((2, 4099), SENTINEL, dtype=torch.int16, device=dev())
    c = torch.full((2, 3), 99, dtype=torch.int64, device=dev())
    sd.launch_torch(y, c)                                                  # warm: nothing is loaded inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sd.launch_torch(y, c)
    y.fill_(SENTINEL)
    c.fill_(99)
    graph.replay()
    torch.cuda.synchronize()
    same(y.cpu().numpy(), want, 'replayed codes')
    same(c.cpu().numpy(), want_counts, 'replayed counts')
    del graph
    sd.close()


def test_plain_c_consumer_samples_to_codes_on_the_device(tmp_path):
    exe = tmp_path / 'sampled_dac_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'sampled_dac_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'wfk_sample_short_dac<16,' in r.stdout and 'parity ok' in r.stdout
