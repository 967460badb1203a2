"""The binned demodulator on the host: the referee (tests/bdemod_ref.py) against a plain double loop, every refusal of
`BinnedDemodulator` that needs no device, the bin-group rule of the library against its Python restatement, and what
plan creation answers without a device.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bdemod_ref as ref
from waveforms_amd import _engine, utils
from waveforms_amd.utils import BinnedDemodulator, getFTMatrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any touch of the library fails the test"""
    def refuse():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_engine, 'lib', refuse)


@pytest.mark.parametrize('dtype', [np.int16, np.float32, np.float64])
def test_referee_against_a_double_loop(dtype):
    rng = np.random.default_rng(5)
    for N, nf, bin, start, bins in ((23, 2, 4, 3, None), (23, 3, 5, 0, 3), (9, 1, 1, 2, None), (12, 2, 12, 0, None),
                                    (40, 5, 7, 4, 4)):
        S = 3
        e = getFTMatrix(rng.uniform(-400e6, 400e6, nf), N, rng.uniform(0, 6.3, nf))
        x = rng.integers(-32768, 32768, (S, N + 2)).astype(np.int16) if dtype == np.int16 else \
            rng.normal(size=(S, N + 2)).astype(dtype)
        W = ref.bins_of(N, bin, start, bins)
        got, want = ref.binned(x, e, bin, start, bins), ref.brute_force(x, e, bin, start, bins)
        assert got.shape == (S, W, nf) and got.dtype == np.complex128
        # two summation orders of one fp64 sum of `bin` rounded products: each is within bin * 2^-53 of SUM |x| |e|
        assert np.all(np.abs(got - want) <= 2 * bin * 2.0 ** -53 * ref.magnitude(x, e, bin, start, bins))
        # the samples outside the bins take no part
        y = x.astype(np.float64)
        y[:, :start] = np.nan
        y[:, start + W * bin:] = np.inf
        assert np.array_equal(ref.binned(y, e, bin, start, bins), got)
    assert [ref.bin_of(k, 4, 3, 5) for k in (0, 2, 3, 6, 7, 22, 23)] == [None, None, 0, 0, 1, 4, None]


def test_referee_is_exact_on_integers():
    rng = np.random.default_rng(6)
    x = rng.integers(-32768, 32768, (4, 50)).astype(np.int16)
    e = rng.integers(-3, 4, (50, 3)) + 1j * rng.integers(-3, 4, (50, 3))
    assert np.array_equal(ref.binned(x, e, 7, 1), ref.brute_force(x, e, 7, 1))


def test_bins_and_refusals_without_a_device(no_library):
    bd = BinnedDemodulator([10e6, 20e6], 1000, bin=128)
    assert (bd.n, bd.nf, bd.start, bd.bin, bd.bins, bd.dtype) == (1000, 2, 0, 128, 7, np.dtype(np.float64))
    assert BinnedDemodulator([10e6], 1000, bin=100, start=3).bins == 9
    assert BinnedDemodulator([10e6], 1000, bin=1000).bins == 1
    assert BinnedDemodulator([10e6], 1000, bin=100, start=3, bins=4, dtype=np.int16).bins == 4
    # weight=None is 2 / bin on every sample; an explicit weight and from_matrix are used as given
    assert np.array_equal(bd.e, getFTMatrix([10e6, 20e6], 1000, weight=np.full(1000, 2 / 128)))
    w = np.linspace(0.5, 1.5, 1000)
    assert np.array_equal(BinnedDemodulator([10e6], 1000, bin=10, weight=w).e, getFTMatrix([10e6], 1000, weight=w))
    e = getFTMatrix([10e6, 20e6, 30e6], 64)
    assert np.array_equal(BinnedDemodulator.from_matrix(e, bin=16, dtype=np.float32).e, e)
    for kwargs, message in ((dict(bin=0), 'bin >= 1'), (dict(bin=-4), 'bin >= 1'), (dict(bin=16, start=-1), 'start >= 0'),
                            (dict(bin=16, bins=0), 'bins >= 1'), (dict(bin=65), 'bins >= 1'),
                            (dict(bin=16, start=64), 'bins >= 1'), (dict(bin=16, start=70), 'bins >= 1'),
                            (dict(bin=16, bins=5), 'exceeds N'), (dict(bin=16, start=1, bins=4), 'exceeds N'),
                            (dict(bin=16, dtype=np.int32), 'trace dtype must be'),
                            (dict(bin=16, dtype=np.complex128), 'trace dtype must be')):
        with pytest.raises(ValueError, match=message):
            BinnedDemodulator.from_matrix(e, **kwargs)
        with pytest.raises(ValueError, match=message):
            BinnedDemodulator([10e6, 20e6, 30e6], 64, **kwargs)
    with pytest.raises(ValueError, match='must be .N, nf.'):
        BinnedDemodulator.from_matrix(e[0], bin=4)
    # an entry of a USED row that is not finite is named; one outside the bins is nobody's business
    bad = e.copy()
    bad[37, 1] = complex(1.0, np.inf)
    with pytest.raises(ValueError, match=r'e\[37, 1\] is not finite'):
        BinnedDemodulator.from_matrix(bad, bin=16)
    bad[20, 2] = np.nan
    with pytest.raises(ValueError, match=r'e\[20, 2\] is not finite'):
        BinnedDemodulator.from_matrix(bad, bin=16)
    BinnedDemodulator.from_matrix(bad, bin=16, start=38, bins=1)
    BinnedDemodulator.from_matrix(bad, bin=4, bins=5)
    # NumPy signals that are refused before anything is sent to a device
    bd = BinnedDemodulator.from_matrix(e, bin=16, dtype=np.int16)
    with pytest.raises(ValueError, match='complex traces'):
        bd(np.zeros(64, dtype=complex))
    with pytest.raises(ValueError, match='does not fit'):
        bd(np.zeros(64))
    with pytest.raises(ValueError, match='shape'):
        bd(np.zeros(63, dtype=np.int16))
    bd.close()                                                        # no plan was made: nothing to release
    assert 'BinnedDemodulator' in utils.__all__


TABLE = [(S, nf, W) for S in (1, 63, 64, 65, 130, 4096, 65536, 65537, 10**6) for nf in (1, 4, 5, 8, 9, 16, 17, 33, 100)
         for W in (1, 2, 3, 4, 5, 7, 8, 32, 40, 63, 256, 4095, 10**5)]


def test_bin_groups_follow_the_documented_rule():
    lib = _engine.lib()
    for S, nf, W in TABLE:
        got = lib.wfk_bdemod_bin_groups(S, nf, W)
        assert got == ref.bin_groups(S, nf, W) == _engine.bdemod_bin_groups(S, nf, W), (S, nf, W, got)
        assert 1 <= got <= max(1, W // 4) and got <= 1024
    # the cases the rule was written for: the flagship fills the chip with one group; few shots spread their bins, four
    # to a group; fewer than four bins stay together
    assert ref.bin_groups(65536, 8, 32) == 1 and ref.bin_groups(65536, 8, 256) == 1
    assert ref.bin_groups(1024, 4, 64) == 16 and ref.bin_groups(1, 8, 4095) == 819 and ref.bin_groups(130, 33, 40) == 10
    assert ref.bin_groups(1, 1, 1) == ref.bin_groups(1, 1, 3) == ref.bin_groups(1, 8, 7) == 1
    for args in ((0, 8, 32), (-1, 8, 32), (64, 0, 32), (64, 8, 0)):
        assert lib.wfk_bdemod_bin_groups(*args) == 0 == ref.bin_groups(*args)
    assert lib.wfk_bdemod_bin_groups(2**62, 2**21, 2**31 - 1) == 1       # nothing overflows on the way


def test_library_refuses_before_any_device_work():
    """the C side's own refusals of a plan come before it looks for a device: WFK_EINVAL (-1) here; a plan that passes
    them is answered WFK_EHIP (-3) where there is no device"""
    lib = _engine.lib()
    h = C.c_void_p()
    e = np.ascontiguousarray(getFTMatrix([10e6, 20e6], 64))
    bad = e.copy()
    bad[21, 1] = np.nan

    def create(m, n, nf, kind, start, bin, bins):
        return lib.wfk_bdemod_plan_create(m.ctypes.data, n, nf, kind, start, bin, bins, C.byref(h))

    for args, message in (((e, 0, 2, 0, 0, 16, 4), b'n_points >= 1'), ((e, 64, 0, 0, 0, 16, 4), b'n_freq'),
                          ((e, 64, 2, 0, 0, 0, 4), b'bin < 1'), ((e, 64, 2, 0, 0, 16, 0), b'bins < 1'),
                          ((e, 64, 2, 0, -1, 16, 4), b'start < 0'), ((e, 64, 2, 0, 1, 16, 4), b'start + bins * bin > n_points'),
                          ((e, 64, 2, 0, 0, 16, 5), b'start + bins * bin > n_points'),
                          ((e, 64, 2, 0, 65, 1, 1), b'start + bins * bin > n_points'),
                          ((e, 64, 2, 0, 0, 2**62, 2**62), b'start + bins * bin > n_points'),
                          ((e, 64, 2, 0, 2**63 - 1, 2**63 - 1, 2**63 - 1), b'start + bins * bin > n_points'),
                          ((e, 2**62, 2, 0, 0, 1, 2**31), b'bins * n_freq exceeds'),
                          ((e, 64, 2, 2, 0, 16, 4), b'in_kind must be'), ((bad, 64, 2, 4, 0, 16, 4), b'e[21, 1] is not finite'),
                          ((bad, 64, 2, 4, 16, 1, 6), b'e[21, 1] is not finite')):
        assert create(*args) == -1 and not h, args[1:]
        assert message in lib.wfk_last_error(), (args[1:], lib.wfk_last_error())
    assert lib.wfk_bdemod_plan_create(None, 64, 2, 0, 0, 16, 4, C.byref(h)) == -1
    assert lib.wfk_bdemod_plan_create(e.ctypes.data, 64, 2, 0, 0, 16, 4, None) == -1
    for m, start, bin, bins in ((e, 0, 16, 4), (bad, 22, 14, 3), (bad, 0, 7, 3)):       # fine: the NaN is in no bin
        rc = create(m, 64, 2, 4, start, bin, bins)
        said = lib.wfk_last_error()
        if _engine.device_count() == 0:
            assert rc == -3 and not h and b'no HIP device' in said
        else:
            assert rc == 0 and h
            assert lib.wfk_bdemod_plan_destroy(h) == 0
            h = C.c_void_p()
    assert lib.wfk_bdemod_apply(None, None, 1, 64, None, 8, None) == -1
    assert b'null plan' in lib.wfk_last_error()
    assert lib.wfk_bdemod_plan_destroy(None) == 0
    assert lib.wfk_bdemod_kernel_name(None, 10) == b''


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_bdemod_plan_create', 'wfk_bdemod_apply', 'wfk_bdemod_bin_groups', 'wfk_bdemod_kernel_name',
                 'wfk_bdemod_plan_destroy'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_bdemod_plan wfk_bdemod_plan;' in src
    assert lib.wfk_abi_version() == 2
