"""The state discriminator on the host: the referee (tests/states_ref.py) against a brute-force double loop, the
shots-per-step arithmetic, every refusal before the library is touched, the library's own refusals before any device
work, the empty answers of classify_points and probabilities on host tensors.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import states_ref as ref
from waveforms_amd import _engine, utils
from waveforms_amd.utils import StateDiscriminator, classify_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')


@pytest.fixture
def no_library(monkeypatch):
    """any touch of the library fails the test"""
    def refuse():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_engine, 'lib', refuse)


def random_case(rng, S, nf, K):
    centres = rng.normal(size=(nf, K)) + 1j * rng.normal(size=(nf, K))
    if K > 2 and nf > 1:
        centres[nf // 2, K - 1] = NAN                                  # a tone with one state fewer
    state = rng.integers(0, K, (S, nf))
    x = np.nan_to_num(centres[np.arange(nf)[None], state]) + 0.4 * (rng.normal(size=(S, nf)) + 1j * rng.normal(size=(S, nf)))
    special = [NAN, np.inf, -np.inf, 1e300, -0.0, 0.0]
    for i in range(min(S, 6)):
        x[i, i % nf] = complex(special[i], 0.1) if i % 2 else complex(0.1, special[i])
    return x, centres


def test_referee_against_a_double_loop():
    rng = np.random.default_rng(23)
    for case in range(16):
        S, nf, K = int(rng.integers(0, 40)), int(rng.integers(1, 7)), int(rng.integers(2, 9))
        steps, first = int(rng.integers(1, 9)), int(rng.integers(0, 40))
        x, centres = random_case(rng, S, nf, K)
        labels, words, counts, joint = ref.brute_force(x, centres, steps, first)
        got = ref.labels_ref(x, centres)
        assert got.dtype == np.uint8 and np.array_equal(got, labels), case
        assert np.array_equal(ref.counts_ref(got, K, steps, first), counts), case
        assert counts.sum() == S * nf and np.array_equal(counts.sum(axis=(1, 2)) // nf,
                                                         StateDiscriminator(centres, steps).counts_of(S, first)), case
        b = ref.bits_of(K)
        if words is not None:
            assert np.array_equal(ref.words_ref(got, K), words), case
        if joint is not None:
            assert np.array_equal(ref.joint_ref(words, nf * b, steps, first), joint), case
            assert joint.sum() == S
        # accumulate: two blocks cut anywhere give the counts of the whole
        cut = int(rng.integers(0, S + 1))
        a = ref.counts_ref(got[:cut], K, steps, first)
        assert np.array_equal(ref.counts_ref(got[cut:], K, steps, first + cut, a), counts), case


def test_referee_special_values():
    centres = np.array([[1, -1, NAN, NAN], [2 + 2j, 2 + 2j, 0, NAN]])
    x = np.array([[0, 2 + 2j], [-0.0, -0.0], [NAN, complex(0, NAN)], [np.inf, complex(1, -np.inf)], [1e300, 1e300],
                  [0.5, 1 + 1j]])
    labels = ref.labels_ref(x, centres)
    # ties to the lowest state (point 0 between +-1; duplicate centres), -0.0 as 0.0, NaN / Inf / overflow: invalid
    assert labels.tolist() == [[0, 0], [0, 2], [255, 255], [255, 255], [255, 255], [0, 0]]
    assert ref.words_ref(labels, 4).tolist() == [0, 8, -1, -1, -1, 0]
    assert ref.bits_of(2) == 1 and ref.bits_of(3) == ref.bits_of(4) == 2 and ref.bits_of(5) == ref.bits_of(8) == 3
    joint = ref.joint_ref(ref.words_ref(labels, 4), 4, 2, first=1)
    assert joint.shape == (2, 17) and joint[:, -1].tolist() == [1, 2] and joint[1, 0] == 1 and joint[0, 8] == 1
    assert joint[0, 0] == 1 and joint.sum() == 6
    one_bad = np.array([[0, 1, 255], [1, 1, 1]], dtype=np.uint8)
    assert ref.words_ref(one_bad, 2).tolist() == [-1, 7]
    counts = ref.counts_ref(one_bad, 2, 1)
    assert counts.tolist() == [[[1, 1, 0], [0, 2, 0], [0, 1, 1]]]


def test_counts_of(no_library):
    sd = StateDiscriminator([[1, -1]], steps=10)
    assert sd.counts_of(0).tolist() == [0] * 10
    assert sd.counts_of(3).tolist() == [1, 1, 1] + [0] * 7                                    # S < steps
    assert sd.counts_of(3, first=8).tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1, 1]               # across the cycle edge
    assert sd.counts_of(25, first=9).tolist() == [3, 3, 3, 3, 2, 2, 2, 2, 2, 3]
    big = 2**40 + 7                                                                         # (2^40 + 7) % 10 == 3
    assert sd.counts_of(12, first=big).tolist() == [1, 1, 1, 2, 2, 1, 1, 1, 1, 1]
    c = sd.counts_of(2**41 + 5, first=2**40)
    assert c.dtype == np.int64 and int(c.sum()) == 2**41 + 5 and c.max() - c.min() == 1
    for shots, first in ((-1, 0), (1, -1)):
        with pytest.raises(ValueError, match='must not be negative'):
            sd.counts_of(shots, first)
    for S in (0, 1, 9, 10, 11, 1000):
        for first in (0, 1, 9, 53, big):
            want = np.bincount(ref.steps_of_block(S, first, 10), minlength=10)
            assert sd.counts_of(S, first).tolist() == want.tolist(), (S, first)


def test_constructor_refusals(no_library):
    ok = np.ones((3, 2)) * [1, -1]
    for args, message in (((np.ones((3, 1)), ), r'n_states must lie in \[2, 8\]'),
                          ((np.ones((3, 9)), ), r'n_states must lie in \[2, 8\]'),
                          ((np.ones((1025, 2)), ), r'n_tones must lie in \[1, 1024\]'),
                          ((np.ones((0, 2)), ), r'n_tones must lie in \[1, 1024\]'),
                          ((ok, 0), 'steps >= 1'), ((ok, -4), 'steps >= 1'),
                          ((np.ones(4), ), 'centres must be'), ((np.ones((2, 2, 2)), ), 'centres must be'),
                          ((ok, 2**31), 'exceeds'),
                          ((np.array([[1, -1], [NAN, complex(1, NAN)], [0, 1]]), ), 'tone 1: no finite centre')):
        with pytest.raises(ValueError, match=message):
            StateDiscriminator(*args)
        with pytest.raises(ValueError, match=message):
            _engine.StatesPlan(*args)
    sd = StateDiscriminator(np.array([[1, -1, NAN], [0, 1j, 2]]), steps=4)
    assert (sd.nf, sd.n_states, sd.steps, sd.bits, sd.word_bits, sd.joint_bins) == (2, 3, 4, 2, 4, 17)
    assert sd.centres.dtype == np.complex128 and sd.centres.flags.c_contiguous
    assert StateDiscriminator(np.ones((1024, 8))).joint_bins is None
    assert StateDiscriminator(np.ones((8, 4))).joint_bins == 65537 and StateDiscriminator(np.ones((17, 2))).joint_bins is None
    sd.close()                                                        # no plan was made: nothing to release


def test_apply_refusals_on_metadata(no_library):
    """host tensors stand in for device ones (`device=False`), only their metadata is read"""
    nf, K, G, S = 3, 2, 4, 7
    sd = StateDiscriminator(np.ones((nf, K)) * [1, -1], steps=G)
    c128, i64, u8 = torch.complex128, torch.int64, torch.uint8
    x = torch.zeros((S, nf + 8), dtype=c128)[:, 3:3 + nf]
    labels = torch.zeros((S, nf + 5), dtype=u8)[:, 1:1 + nf]
    words, counts, joint = torch.zeros(S, dtype=i64), torch.zeros((G, nf, K + 1), dtype=i64), torch.zeros((G, 9), dtype=i64)
    (xp, xs), (lp, ls), wp, cp, jp = sd.check(x, labels, words, counts, joint, first=5, device=False)
    assert (xp, xs, lp, ls) == (x.data_ptr(), nf + 8, labels.data_ptr(), nf + 5)
    assert (wp, cp, jp) == (words.data_ptr(), counts.data_ptr(), joint.data_ptr())
    assert sd.check(x, None, None, counts, device=False)[1:] == ((None, 0), None, counts.data_ptr(), None)
    with pytest.raises(ValueError, match='first must not be negative'):
        sd.check(x, labels, first=-1, device=False)
    with pytest.raises(ValueError, match='no output'):
        sd.check(x, device=False)
    flat = torch.zeros(S * nf, dtype=c128)
    for bad in (flat.as_strided((S, nf), (nf - 1, 1)), x[:, :nf - 1], x.to(torch.complex64), x.real, x[0], x.t()):
        with pytest.raises(ValueError, match='points must be'):
            sd.check(bad, labels, device=False)
    with pytest.raises(ValueError, match='points must be'):          # without "device=False" a host tensor is refused
        sd.check(x, labels)
    flat8 = torch.zeros(S * nf, dtype=u8)
    for bad in (flat8.as_strided((S, nf), (nf - 1, 1)), labels[:S - 1], labels[:, :nf - 1], labels.to(torch.int8),
                torch.zeros((S, nf + 1), dtype=u8), labels.reshape(-1)):
        with pytest.raises(ValueError, match='labels must be'):
            sd.check(x, bad, device=False)
    for bad in (words[:S - 1], words.to(torch.int32), torch.zeros(2 * S, dtype=i64)[::2], words.view(S, 1)):
        with pytest.raises(ValueError, match='words must be'):
            sd.check(x, None, bad, device=False)
    for bad in (counts[:G - 1], counts.to(torch.int32), torch.zeros((G, nf, K + 2), dtype=i64)[:, :, :K + 1],
                counts.view(G, -1), torch.zeros((G, nf, K), dtype=i64)):
        with pytest.raises(ValueError, match='counts must be'):
            sd.check(x, None, None, bad, device=False)
    for bad in (joint[:G - 1], joint.to(torch.float64), torch.zeros((G, 10), dtype=i64)[:, :9], torch.zeros((G, 8), dtype=i64)):
        with pytest.raises(ValueError, match='joint must be'):
            sd.check(x, None, None, None, bad, device=False)
    # the word and the joint table have their widths
    wide = StateDiscriminator(np.ones((17, 2)) * [1, -1])                       # 17 bits: words, no joint
    xw = torch.zeros((S, 17), dtype=c128)
    wide.check(xw, None, words, device=False)
    with pytest.raises(ValueError, match='joint needs nf \\* bits <= 16, got 17'):
        wide.check(xw, None, None, None, torch.zeros((1, 9), dtype=i64), device=False)
    wider = StateDiscriminator(np.ones((21, 5)))                                # 63 bits
    with pytest.raises(ValueError, match='words need nf \\* bits <= 62, got 63'):
        wider.check(torch.zeros((S, 21), dtype=c128), None, words, device=False)
    # overlaps between every pair of sides: one arena of bytes, viewed per side
    arena = torch.zeros(1 << 16, dtype=u8)

    def at(offset, dtype, shape):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return arena[offset:offset + n].view(dtype).view(shape)

    homes = {'points': (0, c128, (S, nf)), 'labels': (4096, u8, (S, nf)), 'words': (8192, i64, (S, )),
             'counts': (12288, i64, (G, nf, K + 1)), 'joint': (16384, i64, (G, 9))}
    order = list(homes)
    good = {name: at(*home) for name, home in homes.items()}
    sd.check(good['points'], good['labels'], good['words'], good['counts'], good['joint'], device=False)
    behind = at(S * nf * 16, u8, (S, nf))                                       # adjacent to the points: fine
    sd.check(good['points'], behind, device=False)
    for i, early in enumerate(order):
        for late in order[i + 1:]:
            sides = dict(good)
            offset, _, _ = homes[early]
            _, dtype, shape = homes[late]
            sides[late] = at(offset + 16, dtype, shape)                         # the later side laid over the earlier one
            with pytest.raises(ValueError, match='out of place: %s overlaps %s' % (late, early)):
                sd.check(sides['points'], sides['labels'], sides['words'], sides['counts'], sides['joint'], device=False)
    # between the rows of strided points is still inside their extent; no shots: no points to overlap
    widep = at(0, c128, (S, 2 * nf))
    inside = widep[:, nf:].view(torch.int64)[:G * nf * (K + 1) // (2 * nf), :2 * nf]
    assert inside.data_ptr() == widep.data_ptr() + nf * 16
    lab_inside = arena[nf * 16:nf * 16 + S * nf].view(S, nf)
    with pytest.raises(ValueError, match='labels overlaps points'):
        sd.check(widep[:, :nf], lab_inside, device=False)
    sd.check(widep[:0, :nf], lab_inside[:0], None, good['counts'], device=False)
    with pytest.raises(ValueError, match='accumulate=True needs'):
        sd.apply_torch(good['points'], good['labels'], accumulate=True)
    with pytest.raises(ValueError, match='accumulate=True needs'):
        sd.apply_torch(good['points'], None, good['words'], accumulate=True)


def test_library_refuses_before_any_device_work():
    """the C side's own refusals of a plan come before it looks for a device: WFK_EINVAL (-1) here"""
    lib = _engine.lib()
    h = C.c_void_p()
    c = np.ascontiguousarray(np.ones((4, 8)) * np.arange(8), dtype=np.complex128)
    allnan = c[:, :2].copy()
    allnan[2] = NAN
    for args, message in (((c.ctypes.data, 0, 2, 1), b'n_tones must lie in [1, 1024]'),
                          ((c.ctypes.data, 1025, 2, 1), b'n_tones must lie in [1, 1024]'),
                          ((c.ctypes.data, 4, 1, 1), b'n_states must lie in [2, 8]'),
                          ((c.ctypes.data, 4, 9, 1), b'n_states must lie in [2, 8]'),
                          ((c.ctypes.data, 4, 2, 0), b'steps < 1'), ((c.ctypes.data, 4, 2, -3), b'steps < 1'),
                          ((c.ctypes.data, 4, 2, 2**31), b'too large'), ((None, 4, 2, 1), b'null centres'),
                          ((allnan.ctypes.data, 4, 2, 1), b'tone 2: no finite centre')):
        assert lib.wfk_states_plan_create(*args, C.byref(h)) == -1 and not h, args
        assert message in lib.wfk_last_error(), (args, lib.wfk_last_error())
    assert lib.wfk_states_plan_create(c.ctypes.data, 4, 2, 1, None) == -1
    assert lib.wfk_states_apply(None, None, 1, 4, 0, None, 4, None, None, None, 0, None) == -1
    assert b'null plan' in lib.wfk_last_error()
    assert lib.wfk_states_plan_destroy(None) == 0
    assert lib.wfk_states_kernel_name(None, 10) == b''


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_states_plan_create', 'wfk_states_apply', 'wfk_states_kernel_name', 'wfk_states_plan_destroy'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_states_plan wfk_states_plan;' in src
    assert lib.wfk_abi_version() == 2
    assert (_engine.STATES_MAX_TONES, _engine.STATES_MAX_STATES) == (1024, 8)
    assert '#define WFK_STATES_MAX_TONES 1024' in src and '#define WFK_STATES_MAX_STATES 8' in src


def test_classify_points_without_a_device(no_library):
    centres = np.array([[1, -1, 1j], [0, 2, NAN]])
    for shape in ((0, 2), (3, 0, 2), (0, 0, 2)):
        labels = classify_points(np.zeros(shape, dtype=complex), centres)
        assert labels.shape == shape and labels.dtype == np.uint8
        labels, counts = classify_points(np.zeros(shape, dtype=complex), centres, steps=3, return_counts=True)
        assert labels.shape == shape and counts.shape == (3, 2, 4) and counts.dtype == np.int64 and not counts.any()
    with pytest.raises(ValueError, match='shape'):
        classify_points(np.zeros((4, 3), dtype=complex), centres)
    with pytest.raises(ValueError, match='steps >= 1'):
        classify_points(np.zeros((0, 2), dtype=complex), centres, steps=0)
    assert 'StateDiscriminator' in utils.__all__ and 'classify_points' in utils.__all__


def test_probabilities_and_calibration_on_the_host():
    """probabilities and from_calibration are plain torch: they run on host tensors as well"""
    sd = StateDiscriminator([[1, -1]], steps=3)
    counts = torch.tensor([[[3, 1, 0]], [[1, 0, 1]], [[0, 0, 0]]], dtype=torch.int64)
    p = sd.probabilities(counts, np.array([4, 2, 0]))
    assert p.dtype == torch.float64 and tuple(p.shape) == (3, 1, 2)
    assert p[:2].tolist() == [[[0.75, 0.25]], [[0.5, 0.0]]] and torch.isnan(p[2]).all()
    # shots cycle through three prepared states, one shot of the cycle before the block
    cal = torch.tensor([[1 + 1j, 10], [2 + 0j, 20], [3 - 1j, 30], [1 + 3j, 12], [2 + 2j, 22], [3 + 1j, 32]], dtype=torch.complex128)
    sd3 = StateDiscriminator.from_calibration(cal, 3, first=1, steps=5)
    assert sd3.steps == 5 and sd3.centres.shape == (2, 3)
    assert np.array_equal(sd3.centres, np.array([[3 + 0j, 1 + 2j, 2 + 1j], [31, 11, 21]]))
    assert np.array_equal(StateDiscriminator.from_calibration(cal.numpy(), 3, first=1).centres, sd3.centres)
    missing = StateDiscriminator.from_calibration(cal[:2], 3)                      # no shot of state 2: a NaN centre
    assert np.isnan(missing.centres[:, 2]).all() and np.array_equal(missing.centres[:, :2], cal[:2].numpy().T)
    with pytest.raises(ValueError, match='n_states'):
        StateDiscriminator.from_calibration(cal, 1)
    with pytest.raises(ValueError, match='points must be'):
        StateDiscriminator.from_calibration(cal.real, 2)
