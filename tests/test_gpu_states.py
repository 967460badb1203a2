"""The state discriminator on the device (utils.StateDiscriminator, csrc/wfk_states.hip) against the referee
tests/states_ref.py.  Every output is an integer: labels, words, counts and the joint histogram are compared bit for bit
and count for count, there is no tolerance anywhere."""
import contextlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import states_ref as ref
from graph_replay import eager, replay, sentinels_left
from row_windows import EXTRA, LEFT, Window, bits_equal
from waveforms_amd.utils import Demodulator, StateDiscriminator, classify_points

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS = [1, 63, 64, 65, 257, 1025, 70001]          # the edges of a lane, a wave, a workgroup's block
NFS = [1, 3, 8, 33, 65]
KS = [2, 3, 4, 5, 8]                            # the template K and one below / above it
FIRSTS = [0, 5, 2**40 + 3]
NAN = float('nan')
JOINT_MAX = 1 << 22                             # a joint table is asked for up to this many entries
SENTINEL64 = 0x7FF8A5A5A5A5A5A5
SENTINEL8 = 0xA5                                # no label: labels are 0 .. 7 and 255


def dev():
    return torch.device('cuda', torch.cuda.current_device())


@contextlib.contextmanager
def forced_counters(where):
    """WFK_STATES_COUNTERS, read when a plan is made"""
    old = os.environ.get('WFK_STATES_COUNTERS')
    if where:
        os.environ['WFK_STATES_COUNTERS'] = where
    try:
        yield
    finally:
        if old is None:
            os.environ.pop('WFK_STATES_COUNTERS', None)
        else:
            os.environ['WFK_STATES_COUNTERS'] = old


def discriminator(centres, steps, where):
    """a discriminator whose device plan is made -- and the switch read -- while WFK_STATES_COUNTERS is `where`"""
    with forced_counters(where):
        sd = StateDiscriminator(centres, steps)
        assert ' counts:global' in sd.kernel_name(1) or where != 'global'
    return sd


def make_centres(seed, nf, K):
    """K centres per tone; with K > 2 every third tone has one state fewer and its row padded with NaN"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(nf, K)) + 1j * rng.normal(size=(nf, K))
    if K > 2:
        centres[1::3, K - 1] = NAN
    return centres


def make_points(seed, S, nf, centres):
    """shots near the centre of a random state, the noise wide enough that every state turns up everywhere; a NaN, an
    Inf, a far point and both zeros sprinkled in"""
    rng = np.random.default_rng(seed)
    state = rng.integers(0, centres.shape[1], (S, nf))
    x = np.nan_to_num(centres[np.arange(nf)[None], state]) + 0.5 * (rng.normal(size=(S, nf)) + 1j * rng.normal(size=(S, nf)))
    for i, v in enumerate((complex(NAN, 0.0), complex(0.0, np.inf), 1e300 + 0j, complex(-0.0, -0.0), 0j)):
        x[(11 * i + 3)::997, (i * 2) % nf] = v
    return x


def rule(entries, where):
    return 'lds' if entries <= 4096 and where != 'global' else 'global'


def tile_rule(S, nf):
    tile = 4096
    while tile > 1024 and S * nf // tile < 1024:
        tile //= 2
    return tile


def garbage(shape, dtype=torch.int64):
    return torch.full(shape, 0x5a5a5a5a5a5a if dtype == torch.int64 else SENTINEL8, dtype=dtype, device=dev())


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('nf', NFS)
def test_shapes_steps_and_counters(nf, K):
    """every S, steps, first and both settings of the counter switch for one (nf, K): labels, words (where nf * bits <=
    62), counts and joint (where nf * bits <= 16 and the table is small) from garbage-filled outputs"""
    b = ref.bits_of(K)
    centres = make_centres(100 * nf + K, nf, K)
    x = make_points(nf + K, max(SS), nf, centres)
    xd = torch.from_numpy(x).to(dev())
    want_labels = ref.labels_ref(x, centres)
    assert (want_labels == 255).any() and all((want_labels == k).any() for k in range(K))
    labels_d = torch.from_numpy(want_labels).to(dev())
    want_words = ref.words_ref(want_labels, K) if nf * b <= 62 else None
    words_d = None if want_words is None else torch.from_numpy(want_words).to(dev())
    for where in ('lds', 'global'):
        for S in SS:
            labels = garbage((S, nf), torch.uint8)
            words = None if want_words is None else garbage((S, ))
            for steps in (1, 2, 7, S + 3):
                with forced_counters(where):
                    sd = StateDiscriminator(centres, steps)
                    bins = sd.joint_bins if sd.joint_bins and steps * sd.joint_bins <= JOINT_MAX else None
                    name = 'states_block<%d> tile=%d counts:%s joint:%s' % (
                        2 if K == 2 else 4 if K <= 4 else 8, tile_rule(S, nf), rule(steps * nf * (K + 1), where),
                        'none' if sd.joint_bins is None else rule(steps * sd.joint_bins, where))
                    assert sd.kernel_name(S) == name, (sd.kernel_name(S), name)
                for first in FIRSTS:
                    what = f'nf={nf} K={K} S={S} steps={steps} first={first} counters={where}'
                    labels.fill_(SENTINEL8)
                    counts = garbage((steps, nf, K + 1))
                    joint = None if bins is None else garbage((steps, bins))
                    wrote = sd.apply_torch(xd[:S], labels, words, counts, joint, first=first)
                    assert wrote[0] is labels and wrote[-1] is (counts if joint is None else joint)
                    assert torch.equal(labels, labels_d[:S]), what + ' (labels)'
                    if words is not None:
                        assert torch.equal(words, words_d[:S]), what + ' (words)'
                    want = ref.counts_ref(want_labels[:S], K, steps, first)
                    assert torch.equal(counts, torch.from_numpy(want).to(dev())), what + ' (counts)'
                    if joint is not None:
                        want = ref.joint_ref(want_words[:S], nf * b, steps, first)
                        assert torch.equal(joint, torch.from_numpy(want).to(dev())), what + ' (joint)'
                sd.close()
    assert rule(4096, 'lds') == 'lds' and rule(4097, 'lds') == 'global' and rule(3, 'global') == 'global'


def test_counter_rule_without_the_switch():
    """the rule is a function of the plan's shape alone: 4096 entries are counted in LDS, 4097 are not"""
    with forced_counters(None):
        os.environ.pop('WFK_STATES_COUNTERS', None)
        for steps, nf, K, counts, joint in ((1, 8, 2, 'lds', 'lds'), (455, 1, 7, 'lds', 'lds'), (512, 1, 7, 'lds', 'global'),
                                            (513, 1, 7, 'global', 'global'), (1, 12, 2, 'lds', 'global'),
                                            (1, 17, 2, 'lds', 'none'), (101, 32, 3, 'global', 'none')):
            sd = StateDiscriminator(np.ones((nf, K)) * np.arange(K), steps)
            assert sd.kernel_name(1 << 20).endswith(' counts:%s joint:%s' % (counts, joint)), sd.kernel_name(1 << 20)
            sd.close()
        sd = StateDiscriminator(np.ones((8, 2)) * [1, -1])
        # the block: 4096 points, halved down to 1024 while the launch has fewer than 1024 workgroups
        assert [sd.kernel_name(S).split()[1] for S in (1 << 20, 1 << 19, (1 << 19) - 1, 1 << 18, (1 << 18) - 1, 1 << 17, 1, 0)] == [
            'tile=4096', 'tile=4096', 'tile=2048', 'tile=2048', 'tile=1024', 'tile=1024', 'tile=1024', 'tile=1024']
        sd.close()


def test_accumulate_across_blocks_cut_mid_cycle():
    """blocks of 388, 0, 3 (shorter than the 7 steps) and 609 shots, cut inside a cycle: the first overwrites garbage, the
    others add, with `first` = the shots already taken; and the same onto a random base"""
    nf, K, steps, S = 8, 3, 7, 1000
    centres = make_centres(5, nf, K)
    x = make_points(6, S, nf, centres)
    xd = torch.from_numpy(x).to(dev())
    want_labels = ref.labels_ref(x, centres)
    want_words = ref.words_ref(want_labels, K)
    cuts = [0, 388, 388, 391, S]
    for where in ('lds', 'global'):
        sd = discriminator(centres, steps, where)
        assert sd.joint_bins == 2**16 + 1
        for start in (0, 2**40 + 3):
            counts, joint = garbage((steps, nf, K + 1)), garbage((steps, sd.joint_bins))
            base = torch.randint(-2**40, 2**40, (steps, nf, K + 1), dtype=torch.int64, device=dev())
            base_j = torch.randint(-2**40, 2**40, (steps, sd.joint_bins), dtype=torch.int64, device=dev())
            onto, onto_j = base.clone(), base_j.clone()
            for k in range(4):
                block = xd[cuts[k]:cuts[k + 1]]
                sd.apply_torch(block, counts=counts, joint=joint, first=start + cuts[k], accumulate=k > 0)
                sd.apply_torch(block, counts=onto, joint=onto_j, first=start + cuts[k], accumulate=True)
                upto = cuts[k + 1]
                want = ref.counts_ref(want_labels[:upto], K, steps, start)
                want_j = ref.joint_ref(want_words[:upto], 16, steps, start)
                assert np.array_equal(counts.cpu().numpy(), want), (where, start, k)
                assert np.array_equal(joint.cpu().numpy(), want_j), (where, start, k)
            assert np.array_equal(onto.cpu().numpy(), base.cpu().numpy() + want)
            assert np.array_equal(onto_j.cpu().numpy(), base_j.cpu().numpy() + want_j)
            assert int(counts.sum()) == S * nf and int(joint.sum()) == S
            # a block of no shots, overwriting: every step is without a shot and gets 0
            sd.apply_torch(xd[:0], counts=counts, joint=joint)
            assert not counts.any() and not joint.any()
        sd.close()


def test_rounding_is_unfused():
    """4000 points on the perpendicular bisector of two centres: the two distances agree to the last bits, so the
    rounding decides.  The fused form fma(dr, dr, di * di), emulated exactly with fractions, picks the other state for
    more than 100 of them; the device agrees with the unfused referee on all 4000."""
    centres = np.array([[0.3 + 0.2j, -0.5 + 0.7j]])
    t = np.random.default_rng(7).uniform(-1, 1, 4000)
    mid, along = (centres[0, 0] + centres[0, 1]) / 2, (centres[0, 1] - centres[0, 0]) * 1j
    x = (mid + t * along).reshape(-1, 1)

    def fused(p, c):
        dr, di = float(p.real) - float(c.real), float(p.imag) - float(c.imag)
        return float(Fraction(dr) * Fraction(dr) + Fraction(di * di))          # one rounding of dr^2 + fl(di^2)

    fused_labels = np.array([1 if fused(p, centres[0, 1]) < fused(p, centres[0, 0]) else 0 for p in x[:, 0]], dtype=np.uint8)
    want = ref.labels_ref(x, centres)[:, 0]
    flips = int((fused_labels != want).sum())
    print('points a fused multiply-add would label otherwise:', flips, 'of', len(t))
    assert flips >= 100, flips
    sd = StateDiscriminator(centres)
    got = sd.apply_torch(torch.from_numpy(x).to(dev())).cpu().numpy()[:, 0]
    print('device differs from the unfused referee on', int((got != want).sum()), 'and from the fused form on',
          int((got != fused_labels).sum()))
    assert np.array_equal(got, want)
    sd.close()


def test_special_values():
    inf = np.inf
    centres = np.array([[1, -1, NAN, NAN], [2 + 2j, 2 + 2j, 0, NAN], [0.5, 1j, -1j, -0.5]])
    x = np.array([[0, 2 + 2j, 0.5],                        # an exact tie between +1 and -1; duplicate centres: the lowest
                  [complex(-0.0, -0.0), complex(-0.0, 0.0), complex(0.0, -0.0)],
                  [complex(NAN, 0), 0, 0.5], [0, complex(0, NAN), 0.5], [0, 0, complex(NAN, NAN)],
                  [complex(inf, 0), 0, 0.5], [0, complex(0, -inf), 0.5], [0, 0, complex(-inf, inf)],
                  [1e300, 0, 0.5], [0, complex(0, -1e300), 0.5],       # the distance overflows
                  [1e154, 0, 0.5],                                     # ... and here it does not: (1e154)^2 is finite
                  [0.9, 1, 1j]])
    want = ref.labels_ref(x, centres)
    assert want[0].tolist() == [0, 0, 0] and want[1].tolist() == [0, 2, 0] and want[8].tolist() == [255, 2, 0]
    assert want[10].tolist() == [0, 2, 0] and want[11].tolist() == [0, 2, 1]
    assert [(row == 255).sum() for row in want] == [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    want_words = ref.words_ref(want, 4)
    assert want_words.tolist() == [0, 8, -1, -1, -1, -1, -1, -1, -1, -1, 8, 24]
    for where in ('lds', 'global'):
        sd = discriminator(centres, 2, where)
        labels, words, counts, joint = sd.apply_torch(torch.from_numpy(x).to(dev()), garbage((12, 3), torch.uint8),
                                                      garbage((12, )), garbage((2, 3, 5)), garbage((2, 65)), first=1)
        assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(words.cpu().numpy(), want_words)
        assert np.array_equal(counts.cpu().numpy(), ref.counts_ref(want, 4, 2, 1))
        j = joint.cpu().numpy()
        assert np.array_equal(j, ref.joint_ref(want_words, 6, 2, 1))
        # a shot with one invalid tone lands in the last bin and nowhere else
        assert j[:, -1].tolist() == [4, 4] and j[:, :-1].sum() == 4 and j[1, 0] == 1 and j[0, 8] == 1 and j[1, 8] == 1
        sd.close()
    # the NumPy door: leading axes flattened, counts from step 0
    labels, counts = classify_points(x.reshape(3, 4, 3), centres, steps=5, return_counts=True)
    assert labels.shape == (3, 4, 3) and np.array_equal(labels.reshape(12, 3), want)
    assert np.array_equal(counts, ref.counts_ref(want, 4, 5))
    assert np.array_equal(classify_points(x[0], centres), want[0])


class ByteWindow:
    """`Window` for one-byte elements (row_windows.Window takes none): rows of n uint8 inside a wider tensor filled
    with a byte no label takes, at an odd element offset and an odd row stride"""

    def __init__(self, rows, n):
        self.rows, self.n = rows, n
        self.wide = torch.full((rows + 2, n + EXTRA), SENTINEL8, dtype=torch.uint8, device=dev())
        self.win = self.wide[1:1 + rows, LEFT:LEFT + n]

    def assert_guards(self):
        hit = self.wide != SENTINEL8
        hit[1:1 + self.rows, LEFT:LEFT + self.n] = False
        assert not bool(hit.any()), torch.nonzero(hit)[:6].cpu().tolist()


@pytest.mark.parametrize('S', [50, 1500])
@pytest.mark.parametrize('nf,K', [(1, 2), (5, 3), (16, 2), (65, 8)])
def test_row_windows(nf, K, S):
    """points and labels as windows of wider tensors at an odd element offset and an odd row stride: the labels are the
    referee's, every guard keeps its sentinel, the points are bit for bit what they were"""
    steps, first = 3, 4
    centres = make_centres(S + nf, nf, K)
    x = make_points(S, S, nf, centres)
    want = ref.labels_ref(x, centres)
    src, dst = Window(S, nf, np.complex128, x), ByteWindow(S, nf)
    sd = StateDiscriminator(centres, steps)
    wide_counts = torch.full((steps * nf * (K + 1) + 2 * EXTRA, ), SENTINEL64, dtype=torch.int64, device=dev())
    counts = wide_counts[EXTRA:-EXTRA].view(steps, nf, K + 1)
    wide_words = torch.full((S + 2 * EXTRA, ), SENTINEL64, dtype=torch.int64, device=dev())
    words = wide_words[EXTRA:-EXTRA] if nf * sd.bits <= 62 else None
    sd.apply_torch(src.win, dst.win, words, counts, first=first)
    assert np.array_equal(dst.win.cpu().numpy(), want), (nf, K, S)
    assert np.array_equal(counts.cpu().numpy(), ref.counts_ref(want, K, steps, first))
    dst.assert_guards()
    assert bool((wide_counts[:EXTRA] == SENTINEL64).all()) and bool((wide_counts[-EXTRA:] == SENTINEL64).all())
    if words is not None:
        assert np.array_equal(words.cpu().numpy(), ref.words_ref(want, K))
    assert bool((wide_words[:EXTRA] == SENTINEL64).all()) and bool((wide_words[-EXTRA:] == SENTINEL64).all())
    src.assert_holds(x)
    # the labels alone, allocated by the apply, from the same window
    alone = sd.apply_torch(src.win)
    assert isinstance(alone, torch.Tensor) and alone.dtype == torch.uint8 and np.array_equal(alone.cpu().numpy(), want)
    sd.close()


def test_refused_tensors_on_the_device():
    nf, K, G, S = 4, 2, 2, 6
    sd = StateDiscriminator(np.ones((nf, K)) * [1, -1], steps=G)
    arena = torch.zeros(1 << 14, dtype=torch.uint8, device=dev())
    x = arena[:S * nf * 16].view(torch.complex128).view(S, nf)
    labels = arena[4096:4096 + S * nf].view(S, nf)
    words = arena[6144:6144 + S * 8].view(torch.int64)
    counts = arena[8192:8192 + G * nf * 3 * 8].view(torch.int64).view(G, nf, 3)
    joint = arena[10240:10240 + G * 17 * 8].view(torch.int64).view(G, 17)
    sd.apply_torch(x, labels, words, counts, joint)
    with pytest.raises(ValueError, match='labels overlaps points'):
        sd.apply_torch(x, arena[S * nf * 16 - 1:S * nf * 16 - 1 + S * nf].view(S, nf))
    with pytest.raises(ValueError, match='joint overlaps counts'):
        sd.apply_torch(x, None, None, counts, arena[8192 + 8:8192 + 8 + G * 17 * 8].view(torch.int64).view(G, 17))
    with pytest.raises(ValueError, match='labels must be'):
        sd.apply_torch(x, labels.cpu())
    with pytest.raises(ValueError, match='first must not be negative'):
        sd.apply_torch(x, labels, first=-2)
    # the library's own refusals, through the raw pointers: nothing is launched
    X, L, W, Cn, J = x.data_ptr(), labels.data_ptr(), words.data_ptr(), counts.data_ptr(), joint.data_ptr()
    for args, message in (((None, S, nf, 0, L, nf), 'null points / labels'), ((X, S, nf - 1, 0, L, nf), 'points row stride smaller'),
                          ((X, S, nf, 0, L, nf - 1), 'labels row stride smaller'), ((X, S, nf, -1, L, nf), 'first < 0'),
                          ((X, -1, nf, 0, L, nf), 'n_shots < 0'), ((X, S, nf, 0), 'no output'),
                          ((X + 8, S, nf, 0, L, nf), 'not aligned to their element'),
                          ((X, S, nf, 0, None, 0, W + 4), 'not aligned to their element'),
                          ((X, S, nf, 0, X + 16, nf), 'labels overlaps points'), ((X, S, nf, 0, L, nf, L), 'words overlaps labels'),
                          ((X, S, nf, 0, L, nf, W, X), 'counts overlaps points'), ((X, S, nf, 0, L, nf, W, W), 'counts overlaps words'),
                          ((X, S, nf, 0, L, nf, W, Cn, Cn + 8), 'joint overlaps counts'),
                          ((X, S, nf, 0, None, 0, None, None, X), 'joint overlaps points'),
                          ((None, 0, nf, 0, None, 0, None, Cn, Cn), 'joint overlaps counts')):
        with pytest.raises(RuntimeError, match=message):
            sd.plan.apply(*args)
    wide = StateDiscriminator(np.ones((21, 5)) * np.arange(5))                        # 63 bits: no words, no joint
    xw = torch.zeros((S, 21), dtype=torch.complex128, device=dev())
    with pytest.raises(RuntimeError, match='words need n_tones \\* bits <= 62'):
        wide.plan.apply(xw.data_ptr(), S, 21, 0, None, 0, W)
    with pytest.raises(RuntimeError, match='joint needs n_tones \\* bits <= 16'):
        wide.plan.apply(xw.data_ptr(), S, 21, 0, None, 0, None, None, J)
    counts.fill_(7)
    sd.plan.apply(None, 0, nf, 0, None, 0, None, Cn)              # no shots: the points are not looked at, counts zeroed
    torch.cuda.synchronize()
    assert not counts.any()
    sd.close()
    wide.close()


@pytest.mark.parametrize('where', ['lds', 'global'])
@pytest.mark.parametrize('accumulate', [False, True])
def test_graph_replay(accumulate, where):
    """one apply with all four outputs captured and replayed on A, B, A: each replay gives the referee's answer and that
    of an eager twin plan and leaves no sentinel; overwriting, the third equals the first; accumulating, every replay
    reads its base anew"""
    nf, K, steps, S, first = 5, 3, 4, 3000, 2**40 + 3
    centres = make_centres(31, nf, K)
    bins = 2 ** (nf * 2) + 1
    feeds = []
    for seed in (41, 42):
        rng = np.random.default_rng(seed)
        x = make_points(seed, S, nf, centres)
        base = (rng.integers(-2**40, 2**40, (steps, nf, K + 1)), rng.integers(-2**40, 2**40, (steps, bins)))
        feeds.append((x, ) + base if accumulate else (x, ))

    def make():
        sd = discriminator(centres, steps, where)
        x = torch.empty((S, nf), dtype=torch.complex128, device=dev())
        labels, words = torch.empty((S, nf), dtype=torch.uint8, device=dev()), torch.empty(S, dtype=torch.int64, device=dev())
        counts = torch.empty((steps, nf, K + 1), dtype=torch.int64, device=dev())
        joint = torch.empty((steps, bins), dtype=torch.int64, device=dev())
        statics = [x, counts, joint] if accumulate else [x]
        return sd, (lambda: sd.apply_torch(x, labels, words, counts, joint, first=first, accumulate=accumulate)), statics, \
            [labels, words, counts, joint]

    sd, run_, statics, outputs = make()
    twin, trun, tstatics, toutputs = make()
    assert ('counts:' + where) in sd.kernel_name(S)
    got = replay(run_, statics, [feeds[0], feeds[1], feeds[0]], outputs)
    for k, outs in enumerate(got):
        feed = feeds[k % 2]
        for mine, theirs in zip(outs, eager(trun, tstatics, feed, toutputs)):
            assert bits_equal(mine, theirs), k
        labels, words, counts, joint = outs
        want = ref.labels_ref(feed[0], centres)
        assert np.array_equal(labels, want) and np.array_equal(words, ref.words_ref(want, K)), k
        assert sentinels_left(labels) == 0 and sentinels_left(words) == 0 and sentinels_left(counts) == 0, k
        assert np.array_equal(counts, ref.counts_ref(want, K, steps, first, feed[1] if accumulate else None)), k
        assert np.array_equal(joint, ref.joint_ref(words, nf * 2, steps, first, feed[2] if accumulate else None)), k
    assert all(bits_equal(a, b) for a, b in zip(got[0], got[2]))
    sd.close()
    twin.close()


def test_side_stream_equals_default_stream():
    nf, K, steps, S = 8, 2, 3, 20000
    centres = make_centres(9, nf, K)
    xd = torch.from_numpy(make_points(9, S, nf, centres)).to(dev())
    sd = StateDiscriminator(centres, steps)

    def run():
        return sd.apply_torch(xd, garbage((S, nf), torch.uint8), garbage((S, )), garbage((steps, nf, K + 1)),
                              garbage((steps, 257)), first=1)

    a = [t.cpu().numpy() for t in run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = [t.clone() for t in run()]
    side.synchronize()
    assert all(bits_equal(p, q.cpu().numpy()) for p, q in zip(a, b)) and int(a[2].sum()) == S * nf
    sd.close()


def test_loopback_sample_quantise_demodulate_discriminate():
    """two prepared states give two-tone shots of other amplitudes and phases: sampled, turned into DAC codes, repeated
    with noise for 400 shots that cycle through 10 steps (step g was prepared in state g mod 2), demodulated, the
    centres taken from the first 100 shots as a calibration run, every shot assigned: in each step the majority state
    of both tones is the prepared one, and P(1) says the same"""
    import waveforms_amd as wf
    from waveforms_amd._sampling import BatchSampler
    from waveforms_amd.distortion import DacStage
    sr, N, G, S, K = 1e9, 2048, 10, 400, 2
    f = np.array([101, 333]) * sr / N
    chans = [(0.2 + 0.3 * k) * wf.cos(2 * np.pi * f[0], 0.9 * k) + (0.4 - 0.2 * k) * wf.cos(2 * np.pi * f[1], -1.1 * k)
             for k in range(K)]
    y = BatchSampler(chans, ('linspace', 0.0, N / sr, N, False)).launch_torch(
        torch.empty((K, N), dtype=torch.float64, device=dev()))
    dac = DacStage.from_full_scale(1.0, N, batch=K)
    state_codes = dac.apply_torch(y)
    torch.manual_seed(3)
    noise = torch.randint(-3000, 3001, (S, N), dtype=torch.int16, device=dev())
    shots = ((state_codes // 2).repeat(S // K, 1) + noise).contiguous()              # |code| <= 16384 + 3000
    assert shots.dtype == torch.int16
    dm = Demodulator(f, N, sampleRate=sr, dtype=np.int16)
    iq = dm.apply_torch(shots)
    sd = StateDiscriminator.from_calibration(iq[:100], K, steps=G)
    assert sd.centres.shape == (2, K) and np.isfinite(sd.centres.real).all()
    counts = torch.empty((G, 2, K + 1), dtype=torch.int64, device=dev())
    labels, _ = sd.apply_torch(iq, labels=torch.empty((S, 2), dtype=torch.uint8, device=dev()), counts=counts)
    per_step = sd.counts_of(S)
    assert per_step.tolist() == [S // G] * G and not counts[:, :, K].any()
    majority = counts[:, :, :K].argmax(dim=2).cpu().numpy()
    assert np.array_equal(majority, np.stack([np.arange(G) % K] * 2, axis=1)), majority
    p1 = sd.probabilities(counts, per_step)[:, :, 1].cpu().numpy()
    assert np.all((p1 > 0.5) == (np.arange(G)[:, None] % K == 1)), p1
    assert np.array_equal(labels.cpu().numpy(), ref.labels_ref(iq.cpu().numpy(), sd.centres))
    for st in (sd, dm, dac):
        st.close()


def test_plain_c_consumer_counts_two_blocks(tmp_path):
    exe = tmp_path / 'states_smoke'
    libdir = os.path.join(ROOT, 'waveforms_amd', 'csrc')
    subprocess.run(['gcc', '-std=c11', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'states_smoke.c'), '-o', str(exe),
                    '-L', libdir, '-lwfk_hip', '-lm', f'-Wl,-rpath,{libdir}'], check=True)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=torch_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'states_smoke: two blocks discriminated on the device, labels, words and counts exact' in r.stdout, r.stdout
