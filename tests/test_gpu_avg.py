"""The trace averager on the device (utils.TraceAverager, csrc/wfk_avg.hip) against the referee tests/avg_ref.py.
int16 codes are summed in integers: those comparisons are of bits.  float32 / float64 traces are summed in fp64 in a fixed
order: they are held to the recursive-summation bound of avg_ref.bounds (derived, not measured) and to themselves, bit
for bit, on a second apply."""
import contextlib
import os
import subprocess

import numpy as np
import pytest
import torch

import avg_ref as ref
from graph_replay import eager, replay, sentinels_left
from row_windows import EXTRA, LEFT, FarWindow, Window, bits_equal, free_far_arena
from waveforms_amd.utils import Demodulator, TraceAverager, average_traces, getFTMatrix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 7, 8, 9, 511, 512, 513, 4096, 4099]
SS = [0, 1, 2, 63, 64, 65, 1000]
GS = [1, 2, 3, 10, 64, 1001]
SENTINEL64 = 0x7FF8A5A5A5A5A5A5


@pytest.fixture(scope='module', autouse=True)
def far_arena():
    """the far rows' arena goes back to the device when the module is done"""
    yield
    free_far_arena()


def dev():
    return torch.device('cuda', torch.cuda.current_device())


@contextlib.contextmanager
def forced_splits(k):
    """WFK_AVG_SPLITS, read when a plan is made"""
    old = os.environ.get('WFK_AVG_SPLITS')
    os.environ['WFK_AVG_SPLITS'] = str(k)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop('WFK_AVG_SPLITS', None)
        else:
            os.environ['WFK_AVG_SPLITS'] = old


def split_rule(S, G, N, itemsize, forced=0):
    """the documented rule (include/wfk.h, wfk_avg_splits)"""
    if S <= 0:
        return 1
    tiles = -(-N // (256 * 16 // itemsize))
    cap = 1024 // tiles // G
    return max(1, min(cap, forced if forced else -(-S // G) // 32))


def firsts(G):
    return sorted({0, 1, G - 1, 5 * G + 3})


def codes(seed, S, N):
    x = np.random.default_rng(seed).integers(-32768, 32768, (S, N)).astype(np.int16)
    x[::7, ::5] = -32768
    return x


def check_int16(N, forced=0):
    """every S, G and first for one N: overwrite from garbage and accumulate onto random int64 contents; -> {(S, G):
    splits}"""
    x = codes(N, max(SS), N)
    xd = torch.from_numpy(x).to(dev())
    seen = {}
    for G in GS:
        av = TraceAverager(N, steps=G, dtype=np.int16)
        old = torch.randint(-2**62, 2**62, (2, G, N), dtype=torch.int64, device=dev())
        old_h = old.cpu().numpy()
        for S in SS:
            seen[S, G] = av.splits(S)
            assert seen[S, G] == split_rule(S, G, N, 2, forced), (S, G, N, forced, seen[S, G])
            name = 'avg_tile<short,sumsq>' + (' + avg_reduce' if seen[S, G] > 1 else '')
            assert av.kernel_name(S) == name, (av.kernel_name(S), name)
            for first in firsts(G):
                what = f'N={N} S={S} G={G} first={first} forced={forced}'
                want, want_sq = ref.sums_ref(x[:S], G, first)
                total = torch.full((G, N), 0x5a5a5a5a5a5a, dtype=torch.int64, device=dev())
                total_sq = torch.full((G, N), -77, dtype=torch.int64, device=dev())
                res = av.apply_torch(xd[:S], total, total_sq, first=first)
                assert res[0] is total and res[1] is total_sq
                got, got_sq = total.cpu().numpy(), total_sq.cpu().numpy()
                assert got.dtype == np.int64 and np.array_equal(got, want), what
                assert np.array_equal(got_sq, want_sq), what + ' (squares)'
                acc = old.clone()
                av.apply_torch(xd[:S], acc[0], acc[1], first=first, accumulate=True)
                acc_h = acc.cpu().numpy()
                assert np.array_equal(acc_h[0], old_h[0] + want) and np.array_equal(acc_h[1], old_h[1] + want_sq), what
                absent = av.counts(S, first) == 0
                assert bits_equal(acc_h[:, absent], old_h[:, absent]), what + ': a step without a shot was written'
                assert absent.sum() == max(G - S, 0)
        plain = TraceAverager(N, steps=G, dtype=np.int16, sumsq=False)           # the sum alone
        alone = plain.apply_torch(xd[:65], first=3)
        assert isinstance(alone, torch.Tensor) and plain.kernel_name(65).startswith('avg_tile<short>')
        assert np.array_equal(alone.cpu().numpy(), ref.sums_ref(x[:65], G, 3)[0]), f'sum alone N={N} G={G}'
        plain.close()
        av.close()
    return seen


@pytest.mark.parametrize('N', NS)
def test_int16_bits(N):
    seen = check_int16(N)
    if N == 512:
        assert seen[1000, 1] == 31 and seen[1000, 2] == 15 and seen[64, 1] == 2            # several splits
        assert seen[63, 1] == 1 and seen[1000, 64] == 1 and seen[65, 3] == 1              # one
    if N == 4099:
        assert seen[1000, 1] == 31 and seen[1000, 10] == 3 and seen[1000, 64] == 1 and seen[2, 1001] == 1


@pytest.mark.parametrize('N', [n for n in NS if n <= 513])
def test_int16_bits_with_forced_splits(N):
    """three splits whatever the shape (where the workspace has the slots): splits without a shot, S < splits"""
    with forced_splits(3):
        seen = check_int16(N, forced=3)
    assert seen[1, 1] == 3 and seen[2, 64] == 3 and seen[1000, 1001] == 1


@pytest.mark.parametrize('G', [1, 2])
def test_int16_overflow_corner(G):
    """65 537 codes of -32768, then of 32767: past an int32 sum and, at four rows, past a uint32 sum of squares"""
    S, N = 65537, 8
    av = TraceAverager(N, steps=G)
    assert av.splits(S) > 1
    for code in (-32768, 32767):
        x = torch.full((S, N), code, dtype=torch.int16, device=dev())
        total, total_sq = av.apply_torch(x)
        counts = av.counts(S)
        assert counts.tolist() == ([65537] if G == 1 else [32769, 32768])
        want = (counts * code)[:, None] * np.ones(N, dtype=np.int64)
        want_sq = (counts * code * code)[:, None] * np.ones(N, dtype=np.int64)
        if G == 1:
            assert want[0, 0] == (-2147516416 if code < 0 else 2147450879)            # 65 537 * 32767: past 2^31 - 1
            assert want_sq[0, 0] == (65537 * 2**30 if code < 0 else 65537 * 32767**2)
        assert np.array_equal(total.cpu().numpy(), want) and np.array_equal(total_sq.cpu().numpy(), want_sq), (G, code)
    with forced_splits(1):                                   # one workgroup walks all of it
        one = TraceAverager(N, steps=G)
        assert one.splits(S) == 1
        total, total_sq = one.apply_torch(x)
        assert np.array_equal(total.cpu().numpy(), want) and np.array_equal(total_sq.cpu().numpy(), want_sq)
        one.close()
    av.close()


def float_traces(seed, S, N, dtype):
    """mixed signs, magnitudes over six decades: the sums cancel, the bound stays far below the values"""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(S, N)) * 10.0 ** rng.integers(-3, 4, (S, N))).astype(dtype)


def assert_within(got, got_sq, x, G, first, old=None, what=''):
    base = (None, None) if old is None else (old[0], old[1])
    want, want_sq = ref.sums_ref(x, G, first, *base)
    bound, bound_sq = ref.bounds(x, G, first, *base)
    fine = np.isfinite(want) & np.isfinite(want_sq)
    with np.errstate(invalid='ignore'):                      # (inf - inf where a sample is not finite: masked below)
        err = np.abs(got.astype(np.longdouble) - want)
        err_sq = np.abs(got_sq.astype(np.longdouble) - want_sq)
    print(what, 'max err / bound:', float(np.max(err[fine] / np.maximum(bound[fine], np.longdouble(1e-300)), initial=0)),
          float(np.max(err_sq[fine] / np.maximum(bound_sq[fine], np.longdouble(1e-300)), initial=0)))
    assert got.dtype == got_sq.dtype == np.float64
    assert np.all(err[fine] <= bound[fine]), (what, float(np.max(err[fine] - bound[fine])))
    assert np.all(err_sq[fine] <= bound_sq[fine]), (what, float(np.max(err_sq[fine] - bound_sq[fine])))
    return want, want_sq, fine


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_float_bound_and_determinism(dtype):
    """the derived bound |sum - exact| <= (m - 1) 2^-52 SUM|terms|, |sumsq - exact| <= m 2^-52 SUM terms^2 per (step,
    column), overwrite and accumulate, one split and several; a second apply gives the same bits"""
    E = 16 // np.dtype(dtype).itemsize
    for N, steps in ((1, (3, )), (E + 1, (1, 3, 10)), (513, (1, 3, 10)), (1031, (3, ))):
        x = float_traces(N, 1000, N, dtype)
        xd = torch.from_numpy(x).to(dev())
        for G in steps:
            av = TraceAverager(N, steps=G, dtype=dtype)
            old = torch.from_numpy(float_traces(N + G, 2 * G, N, np.float64).reshape(2, G, N)).to(dev())
            old[1].abs_()
            old_h = old.cpu().numpy()
            for S in (0, 1, 2, 65, 1000):
                assert av.splits(S) == split_rule(S, G, N, np.dtype(dtype).itemsize)
                for first in (0, 5 * G + 3):
                    what = f'{np.dtype(dtype)} N={N} G={G} S={S} first={first}'
                    total, total_sq = av.apply_torch(xd[:S], first=first)
                    got, got_sq = total.cpu().numpy(), total_sq.cpu().numpy()
                    assert_within(got, got_sq, x[:S], G, first, what=what)
                    again = av.apply_torch(xd[:S], first=first)
                    assert bits_equal(again[0].cpu().numpy(), got) and bits_equal(again[1].cpu().numpy(), got_sq), what
                    acc = old.clone()
                    av.apply_torch(xd[:S], acc[0], acc[1], first=first, accumulate=True)
                    acc_h = acc.cpu().numpy()
                    assert_within(acc_h[0], acc_h[1], x[:S], G, first, old_h, what + ' accumulate')
                    absent = av.counts(S, first) == 0
                    assert bits_equal(acc_h[:, absent], old_h[:, absent]), what
            assert av.kernel_name(1000) == 'avg_tile<%s,sumsq>' % ('float' if dtype == np.float32 else 'double') + (
                ' + avg_reduce' if av.splits(1000) > 1 else '')
            av.close()
    assert split_rule(1000, 1, 513, 4) > 1 and split_rule(65, 3, 513, 8) == 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('S,forced', [(40, 0), (1000, 0), (40, 3)])
def test_nan_and_inf_stay_in_their_column(dtype, S, forced):
    N, G, first = 777, 3, 2
    x = float_traces(5, S, N, dtype)
    x[7, 100], x[S - 2, 640] = np.nan, -np.inf
    with forced_splits(forced):
        av = TraceAverager(N, steps=G, dtype=dtype)
    total, total_sq = av.apply_torch(torch.from_numpy(x).to(dev()), first=first)
    got, got_sq = total.cpu().numpy(), total_sq.cpu().numpy()
    _, _, fine = assert_within(got, got_sq, x, G, first, what=f'nan {np.dtype(dtype)} S={S}')
    g_nan, g_inf = (first + 7) % G, (first + S - 2) % G
    assert fine.sum() == G * N - 2 and not fine[g_nan, 100] and not fine[g_inf, 640]
    assert np.isnan(got[g_nan, 100]) and np.isnan(got_sq[g_nan, 100])
    assert got[g_inf, 640] == -np.inf and got_sq[g_inf, 640] == np.inf
    assert np.isfinite(np.delete(got.reshape(-1), [g_nan * N + 100, g_inf * N + 640])).all()
    av.close()


def wide_int64(G, N):
    """a guarded int64 output: a sentinel-filled (G + 2, N + EXTRA) tensor, the window at [1:1 + G, LEFT:LEFT + N]"""
    wide = torch.full((G + 2, N + EXTRA), SENTINEL64, dtype=torch.int64, device=dev())
    return wide, wide[1:1 + G, LEFT:LEFT + N]


def int64_guards_intact(wide, G, N):
    hit = wide != SENTINEL64
    hit[1:1 + G, LEFT:LEFT + N] = False
    return not bool(hit.any())


@pytest.mark.parametrize('S', [50, 1000])
@pytest.mark.parametrize('N', [5, 1024, 4101])
def test_row_windows(N, S):
    """traces as windows at an odd element offset and an odd row stride (no 16-byte alignment to lean on, another
    alignment in every row), outputs as windows too: the sums are the referee's and every guard keeps its sentinel"""
    G, first = 3, 4
    for dtype in (np.int16, np.float32, np.float64):
        x = codes(N + S, S, N) if dtype == np.int16 else float_traces(N + S, S, N, dtype)
        src = Window(S, N, dtype, x)
        av = TraceAverager(N, steps=G, dtype=dtype)
        if dtype == np.int16:
            wide, total = wide_int64(G, N)
            wide_sq, total_sq = wide_int64(G, N)
            res = av.apply_torch(src.win, total, total_sq, first=first)
            assert res[0].data_ptr() == total.data_ptr()
            want, want_sq = ref.sums_ref(x, G, first)
            assert np.array_equal(total.cpu().numpy(), want) and np.array_equal(total_sq.cpu().numpy(), want_sq), (N, S)
            assert int64_guards_intact(wide, G, N) and int64_guards_intact(wide_sq, G, N), (N, S)
            av.apply_torch(src.win, total, total_sq, first=first + S, accumulate=True)       # the block once more
            assert np.array_equal(total.cpu().numpy(), want + ref.sums_ref(x, G, first + S)[0])
            assert int64_guards_intact(wide, G, N) and int64_guards_intact(wide_sq, G, N), (N, S)
        else:
            dst, dst_sq = Window(G, N, np.float64), Window(G, N, np.float64)
            av.apply_torch(src.win, dst.win, dst_sq.win, first=first)
            assert_within(dst.host(), dst_sq.host(), x, G, first, what=f'window {np.dtype(dtype)} N={N} S={S}')
            dst.assert_guards()
            dst_sq.assert_guards()
            plain = av.apply_torch(torch.from_numpy(x).to(dev()), first=first)
            # the order of additions does not depend on where the rows lie
            assert bits_equal(plain[0].cpu().numpy(), dst.host()) and bits_equal(plain[1].cpu().numpy(), dst_sq.host())
        src.assert_holds(x)
        av.close()


@pytest.mark.parametrize('dtype', [np.int16, np.float64])
def test_output_row_stride(dtype):
    """sum / sumsq with a row stride of N + 3, on both sides of the split threshold"""
    N, G = 1000, 4
    out_t = torch.int64 if dtype == np.int16 else torch.float64
    av = TraceAverager(N, steps=G, dtype=dtype)
    for S in (30, 1000):
        x = codes(S, S, N) if dtype == np.int16 else float_traces(S, S, N, dtype)
        filler = 123456789 if dtype == np.int16 else -1.5
        wide = torch.full((2, G, N + 3), filler, dtype=out_t, device=dev())
        total, total_sq = av.apply_torch(torch.from_numpy(x).to(dev()), wide[0, :, :N], wide[1, :, :N], first=1)
        assert total.stride(0) == N + 3 and bool((wide[:, :, N:] == filler).all())
        if dtype == np.int16:
            want, want_sq = ref.sums_ref(x, G, 1)
            assert np.array_equal(total.cpu().numpy(), want) and np.array_equal(total_sq.cpu().numpy(), want_sq)
        else:
            assert_within(total.cpu().numpy(), total_sq.cpu().numpy(), x, G, 1, what=f'stride N + 3, S={S}')
    av.close()


@pytest.mark.parametrize('dtype', [np.int16, np.float64])
def test_far_rows(dtype):
    """two shots more than 2^32 elements apart: one step (their sum) and two steps (each its own row)"""
    N = 2 * 2048 + 5
    x = codes(3, 2, N) if dtype == np.int16 else float_traces(3, 2, N, dtype)
    src = FarWindow(N, dtype, x)
    for G in (1, 2):
        av = TraceAverager(N, steps=G, dtype=dtype)
        total, total_sq = av.apply_torch(src.win, first=G - 1)
        torch.cuda.synchronize()
        want, want_sq = ref.sums_ref(x, G, G - 1)
        if dtype == np.int16:
            assert np.array_equal(total.cpu().numpy(), want) and np.array_equal(total_sq.cpu().numpy(), want_sq), G
        else:
            assert_within(total.cpu().numpy(), total_sq.cpu().numpy(), x, G, G - 1, what=f'far rows G={G}')
        av.close()
    src.assert_holds(x)


def test_refused_tensors_on_the_device():
    N, G, S = 64, 2, 6
    av = TraceAverager(N, steps=G, dtype=np.float64)
    arena = torch.zeros(4096, dtype=torch.float64, device=dev())
    x = arena[:S * N].view(S, N)
    total, total_sq = arena[1024:1024 + G * N].view(G, N), arena[2048:2048 + G * N].view(G, N)
    av.apply_torch(x, total, total_sq)
    with pytest.raises(ValueError, match='sum overlaps traces'):
        av.apply_torch(x, arena[S * N - 1:S * N - 1 + G * N].view(G, N), total_sq)
    with pytest.raises(ValueError, match='sumsq overlaps sum'):
        av.apply_torch(x, total, arena[1024 + N:1024 + N + G * N].view(G, N))
    with pytest.raises(ValueError, match='sum must be'):
        av.apply_torch(x, total.cpu(), total_sq)
    with pytest.raises(ValueError, match='first must not be negative'):
        av.apply_torch(x, total, total_sq, first=-2)
    # the library's own refusals, through the raw pointers: nothing is launched
    X, T, Q = x.data_ptr(), total.data_ptr(), total_sq.data_ptr()
    for args, message in (((None, S, N, 0, T, N, Q, N), 'null traces / sum'), ((X, S, N, 0, None, N, Q, N), 'null traces / sum'),
                          ((X, S, N - 1, 0, T, N, Q, N), 'traces row stride smaller'),
                          ((X, S, N, 0, T, N - 1, Q, N), 'sum row stride smaller'),
                          ((X, S, N, 0, T, N, Q, N - 1), 'sumsq row stride smaller'),
                          ((X, S, N, -1, T, N, Q, N), 'first < 0'), ((X, -1, N, 0, T, N, Q, N), 'n_shots < 0'),
                          ((X + 4, S, N, 0, T, N, Q, N), 'not aligned to their element'),
                          ((X, S, N, 0, X + 8 * N, N, Q, N), 'sum overlaps traces'),
                          ((X, S, N, 0, T, N, X, N), 'sumsq overlaps traces'),
                          ((X, S, N, 0, T, N, T + 8, N), 'sumsq overlaps sum'),
                          ((None, 0, N, 0, T, N, T, N), 'sumsq overlaps sum')):
        with pytest.raises(RuntimeError, match=message):
            av.plan.apply(*args)
    av.plan.apply(None, 0, N, 0, T, N, Q, N)                      # no shots: the traces are not looked at
    torch.cuda.synchronize()
    assert not arena[1024:1024 + G * N].any() and not arena[2048:2048 + G * N].any()
    av.close()


CAPTURES = [(np.int16, 40, False), (np.int16, 1000, False), (np.float64, 1000, True), (np.float32, 40, True)]


@pytest.mark.parametrize('dtype,S,accumulate', CAPTURES, ids=lambda v: getattr(v, '__name__', str(v)))
def test_graph_replay(dtype, S, accumulate):
    """one apply with sumsq captured and replayed on A, B, A: each replay gives the bits of an eager twin plan and of
    the referee (int16) and leaves no sentinel; with one split (S = 40) and with several (S = 1000).  An accumulating
    apply reads its base anew on every replay."""
    N, G, first = 700, 2, 3
    out_t = torch.int64 if dtype == np.int16 else torch.float64
    feeds = []
    for seed in (21, 22):
        x = codes(seed, S, N) if dtype == np.int16 else float_traces(seed, S, N, dtype)
        base = float_traces(seed + 7, 2 * G, N, np.float64).reshape(2, G, N)
        feeds.append((x, base[0], np.abs(base[1])) if accumulate else (x, ))

    def make():
        av = TraceAverager(N, steps=G, dtype=dtype)
        x = torch.empty((S, N), dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device=dev())
        total, total_sq = (torch.empty((G, N), dtype=out_t, device=dev()) for _ in range(2))
        statics = [x, total, total_sq] if accumulate else [x]
        return av, (lambda: av.apply_torch(x, total, total_sq, first=first, accumulate=accumulate)), statics, [total, total_sq]

    av, run_, statics, outputs = make()
    twin, trun, tstatics, toutputs = make()
    assert (av.splits(S) > 1) == (S == 1000)
    got = replay(run_, statics, [feeds[0], feeds[1], feeds[0]], outputs)
    for k, (total, total_sq) in enumerate(got):
        feed = feeds[k % 2]
        t_total, t_sq = eager(trun, tstatics, feed, toutputs)
        assert bits_equal(total, t_total) and bits_equal(total_sq, t_sq), k
        assert sentinels_left(total) == 0 and sentinels_left(total_sq) == 0, k
        if dtype == np.int16:
            want, want_sq = ref.sums_ref(feed[0], G, first)
            assert np.array_equal(total, want) and np.array_equal(total_sq, want_sq), k
        else:
            assert_within(total, total_sq, feed[0], G, first, feed[1:] if accumulate else None, what=f'replay {k}')
    av.close()
    twin.close()


def test_loopback_average_then_demodulate():
    """ten steps of two-tone shots, sampled, turned into DAC codes and repeated cyclically for 50 shots with a fixed
    integer offset per shot: averaging first and demodulating the ten mean rows agrees with demodulating all 50 rows
    and averaging the IQ points, within the demodulator's bound 1e-12 (|x| @ |e|) on the rows it was given"""
    import waveforms_amd as wf
    from waveforms_amd._sampling import BatchSampler
    from waveforms_amd.distortion import DacStage
    sr, N, G, S = 1e9, 4096, 10, 50
    f = np.array([101, 1234]) * sr / N
    chans = [(0.2 + 0.05 * g) * wf.cos(2 * np.pi * f[0], 0.3 * g) + 0.3 * wf.cos(2 * np.pi * f[1], -0.2 * g) for g in range(G)]
    y = BatchSampler(chans, ('linspace', 0.0, N / sr, N, False)).launch_torch(
        torch.empty((G, N), dtype=torch.float64, device=dev()))
    dac = DacStage.from_full_scale(1.0, N, batch=G)
    step_codes = dac.apply_torch(y)
    offset = torch.arange(S, dtype=torch.int16, device=dev()) * 7 - 150             # |code| stays below 32767 * 0.9 + 200
    shots = (step_codes.repeat(S // G, 1) + offset[:, None]).contiguous()
    assert shots.dtype == torch.int16 and int(step_codes.abs().max()) < 32000

    av = TraceAverager(N, steps=G, dtype=np.int16)
    total, total_sq = av.apply_torch(shots)
    mean, var = av.finish_torch(total, total_sq, av.counts(S))
    assert mean.dtype == torch.float64 and tuple(mean.shape) == (G, N)
    dm_mean, dm_all = Demodulator(f, N, sampleRate=sr, dtype=np.float64), Demodulator(f, N, sampleRate=sr, dtype=np.int16)
    iq_of_mean = dm_mean.apply_torch(mean).cpu().numpy()
    iq_all = dm_all.apply_torch(shots).cpu().numpy()
    mean_of_iq = iq_all.reshape(S // G, G, len(f)).mean(axis=0)
    bound = 1e-12 * (np.abs(mean.cpu().numpy()) @ np.abs(getFTMatrix(f, N, sampleRate=sr)))
    err = np.abs(iq_of_mean - mean_of_iq)
    print('loop-back max err / bound:', float(np.max(err / bound)))
    assert np.all(err <= bound), float(np.max(err / bound))
    # the shots of a step differ by their offsets alone: the variance is that of five integers 70 apart
    assert np.allclose(var.cpu().numpy(), np.var(np.arange(5) * 70.0), rtol=1e-9, atol=0)
    # and the NumPy door gives the same mean
    host_mean, host_var = average_traces(shots.cpu().numpy(), steps=G, return_var=True)
    assert bits_equal(host_mean, mean.cpu().numpy()) and bits_equal(host_var, var.cpu().numpy())
    for st in (av, dm_mean, dm_all, dac):
        st.close()


def test_side_stream_equals_default_stream():
    N, G, S = 1500, 3, 900
    x = float_traces(9, S, N, np.float32)
    av = TraceAverager(N, steps=G, dtype=np.float32)
    a = [t.cpu().numpy() for t in av.apply_torch(torch.from_numpy(x).to(dev()), first=1)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = [t.clone() for t in av.apply_torch(torch.from_numpy(x).to(dev()), first=1)]
    side.synchronize()
    assert av.splits(S) > 1 and bits_equal(a[0], b[0].cpu().numpy()) and bits_equal(a[1], b[1].cpu().numpy())
    av.close()


def test_plain_c_consumer_averages_two_blocks(tmp_path):
    exe = tmp_path / 'avg_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'avg_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'avg_smoke: two blocks averaged on the device, sums exact' in r.stdout, r.stdout
