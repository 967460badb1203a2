"""The trace averager on the host: the referee (tests/avg_ref.py) against a brute-force double loop, the shots-per-step
arithmetic, every refusal before the library is touched, and the empty answers of average_traces.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import avg_ref as ref
from waveforms_amd import _engine, utils
from waveforms_amd.utils import TraceAverager, average_traces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any touch of the library fails the test"""
    def refuse():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_engine, 'lib', refuse)


@pytest.mark.parametrize('dtype', [np.int16, np.float32, np.float64])
def test_referee_against_a_double_loop(dtype):
    rng = np.random.default_rng(11)
    for case in range(12):
        S, N, G = int(rng.integers(0, 40)), int(rng.integers(1, 7)), int(rng.integers(1, 9))
        first = int(rng.integers(0, 4 * G))
        if dtype == np.int16:
            x = rng.integers(-32768, 32768, (S, N)).astype(np.int16)
        else:
            x = (rng.normal(size=(S, N)) * 10.0 ** rng.integers(-3, 4, (S, N))).astype(dtype)
        want, want_sq = ref.brute_force(x, G, first)
        got, got_sq = ref.sums_ref(x, G, first)
        assert got.dtype == want.dtype and got.shape == (G, N)
        if dtype == np.int16:
            assert np.array_equal(got, want) and np.array_equal(got_sq, want_sq), case
        else:                                              # longdouble both ways, in another order
            mag = np.abs(x.astype(np.longdouble))
            tol = np.longdouble(2.0) ** -60 * max(S, 1)
            assert np.all(np.abs(got - want) <= tol * (mag.sum(axis=0) + 1)), case
            assert np.all(np.abs(got_sq - want_sq) <= tol * ((mag * mag).sum(axis=0) + 1)), case
        assert np.array_equal(ref.counts_ref(S, first, G), TraceAverager(N, G, dtype).counts(S, first)), case
        # accumulate: two blocks cut anywhere give the sums of the whole
        cut = int(rng.integers(0, S + 1))
        a, a_sq = ref.sums_ref(x[:cut], G, first)
        b, b_sq = ref.sums_ref(x[cut:], G, first + cut, a, a_sq)
        if dtype == np.int16:
            assert np.array_equal(b, want) and np.array_equal(b_sq, want_sq), case
        else:
            assert np.all(np.abs(b - want) <= tol * (mag.sum(axis=0) + 1)), case


def test_referee_overflow_corner_and_absent_steps():
    x = np.full((65537, 2), -32768, dtype=np.int16)
    s, q = ref.sums_ref(x, 1)
    assert s.tolist() == [[-2147516416] * 2] and q.tolist() == [[65537 * 2**30] * 2]
    s, q = ref.sums_ref(-1 - x, 1)
    assert s.tolist() == [[65537 * 32767] * 2] and q.tolist() == [[65537 * 32767**2] * 2]      # 2 147 450 879: past 2^31 - 1
    old = np.arange(12, dtype=np.int64).reshape(6, 2) - 7
    s, q = ref.sums_ref(x[:2], 6, 5, old, old * 3)                  # steps 5 and 0 have a shot
    assert np.array_equal(s[1:5], old[1:5]) and np.array_equal(q[1:5], 3 * old[1:5])
    assert s[5, 0] == old[5, 0] - 32768 and s[0, 1] == old[0, 1] - 32768 and q[0, 0] == 3 * old[0, 0] + 2**30


def test_counts(no_library):
    av = TraceAverager(16, steps=10)
    assert av.counts(0).tolist() == [0] * 10
    assert av.counts(3).tolist() == [1, 1, 1] + [0] * 7                                    # S < G
    assert av.counts(3, first=8).tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1, 1]               # across the cycle edge
    assert av.counts(25, first=9).tolist() == [3, 3, 3, 3, 2, 2, 2, 2, 2, 3]
    assert av.counts(10, first=7).tolist() == [1] * 10
    big = 2**40 + 7
    assert av.counts(12, first=big).tolist() == ref.counts_ref(12, big % 10, 10).tolist()
    assert av.counts(12, first=big).tolist() == [1, 1, 1, 2, 2, 1, 1, 1, 1, 1]            # (2^40 + 7) % 10 == 3
    c = av.counts(2**41 + 5, first=2**40)
    assert c.dtype == np.int64 and int(c.sum()) == 2**41 + 5 and c.max() - c.min() == 1
    assert TraceAverager(4, steps=1).counts(2**50, first=2**45).tolist() == [2**50]
    for shots, first in ((-1, 0), (1, -1)):
        with pytest.raises(ValueError, match='must not be negative'):
            av.counts(shots, first)
    for S in (0, 1, 9, 10, 11, 1000):
        for first in (0, 1, 9, 53):
            assert av.counts(S, first).tolist() == ref.counts_ref(S, first, 10).tolist(), (S, first)


def test_constructor_refusals(no_library):
    for args, message in (((0, ), 'n_points >= 1'), ((-3, ), 'n_points >= 1'), ((16, 0), 'steps >= 1'),
                          ((16, -1), 'steps >= 1'), ((16, 1, np.int32), 'trace dtype must be'),
                          ((16, 1, np.complex128), 'trace dtype must be')):
        with pytest.raises(ValueError, match=message):
            TraceAverager(*args)
        with pytest.raises(ValueError, match=message):
            _engine.AvgPlan(*args)
    av = TraceAverager(16, steps=3, dtype=np.float32)
    assert (av.n, av.steps, av.dtype, av.sum_dtype) == (16, 3, np.dtype(np.float32), np.dtype(np.float64))
    assert TraceAverager(16).sum_dtype == np.dtype(np.int64)
    av.close()                                                        # no plan was made: nothing to release


def test_apply_refusals_on_metadata(no_library):
    """stride < N, a negative first, wrong shapes and dtypes, and sum / sumsq overlapping the traces or each other: host
    tensors stand in for device ones (`device=False`), only their metadata is read"""
    N, G, S = 24, 3, 7
    av = TraceAverager(N, steps=G, dtype=np.float64)
    x = torch.zeros((S, N + 8), dtype=torch.float64)[:, 3:3 + N]
    total, total_sq = torch.zeros((G, N), dtype=torch.float64), torch.zeros((G, N + 3), dtype=torch.float64)[:, :N]
    (xp, xs), (sp, ss), (qp, qs) = av.check(x, total, total_sq, first=5, device=False)
    assert (xp, xs, sp, ss, qp, qs) == (x.data_ptr(), N + 8, total.data_ptr(), N, total_sq.data_ptr(), N + 3)
    assert av.check(x, total, None, device=False)[2] == (None, 0)
    with pytest.raises(ValueError, match='first must not be negative'):
        av.check(x, total, total_sq, first=-1, device=False)
    flat = torch.zeros(S * N, dtype=torch.float64)
    for bad in (flat.as_strided((S, N), (N - 1, 1)), x[:, :N - 1], x.to(torch.float32), x[0], x.t(),
                torch.zeros((S, N), dtype=torch.int16)):
        with pytest.raises(ValueError, match='traces must be'):
            av.check(bad, total, total_sq, device=False)
    with pytest.raises(ValueError, match='complex traces'):
        av.check(x.to(torch.complex128), total, device=False)
    for bad in (flat.as_strided((G, N), (N - 1, 1)), total[:2], total[:, :N - 1], total.to(torch.int64),
                torch.zeros((G, N + 1), dtype=torch.float64), total.view(-1)):
        with pytest.raises(ValueError, match='sum must be'):
            av.check(x, bad, total_sq, device=False)
        with pytest.raises(ValueError, match='sumsq must be'):
            av.check(x, total, bad, device=False)
    with pytest.raises(ValueError, match='traces must be'):          # without "device=False" a host tensor is refused
        av.check(x, total)
    # overlap: one arena, the traces in front
    arena = torch.zeros(4096, dtype=torch.float64)
    tr = arena[:S * N].view(S, N)
    behind = arena[S * N:S * N + G * N].view(G, N)                   # adjacent: fine
    after = arena[2048:2048 + G * N].view(G, N)
    av.check(tr, behind, after, device=False)
    inside = arena[S * N - 1:S * N - 1 + G * N].view(G, N)           # one element into the last trace
    with pytest.raises(ValueError, match='out of place: sum overlaps traces'):
        av.check(tr, inside, after, device=False)
    with pytest.raises(ValueError, match='out of place: sumsq overlaps traces'):
        av.check(tr, after, inside, device=False)
    with pytest.raises(ValueError, match='out of place: sumsq overlaps sum'):
        av.check(tr, after, after, device=False)
    with pytest.raises(ValueError, match='out of place: sumsq overlaps sum'):
        av.check(tr, after, arena[2048 + N:2048 + N + G * N].view(G, N), device=False)
    # between the rows of strided traces is still inside their extent
    wide = arena[:S * 2 * N].view(S, 2 * N)
    with pytest.raises(ValueError, match='sum overlaps traces'):
        av.check(wide[:, :N], wide[:G, N:], None, device=False)
    av.check(wide[:0, :N], wide[:G, N:], None, device=False)        # no shots: no traces to overlap
    # int16 traces take int64 sums
    av16 = TraceAverager(N, steps=G)
    codes = torch.zeros((S, N), dtype=torch.int16)
    av16.check(codes, total.to(torch.int64), None, device=False)
    with pytest.raises(ValueError, match='sum must be'):
        av16.check(codes, total, None, device=False)
    with pytest.raises(ValueError, match='accumulate=True needs'):
        av16.apply_torch(codes, None, accumulate=True)


def test_library_refuses_before_any_device_work():
    """the C side's own refusals of a plan come before it looks for a device: WFK_EINVAL (-1) here"""
    lib = _engine.lib()
    h = C.c_void_p()
    for args, message in (((0, 1, 4), b'n_points < 1'), ((-5, 1, 4), b'n_points < 1'), ((16, 0, 4), b'steps < 1'),
                          ((16, -2, 0), b'steps < 1'), ((16, 1, 2), b'in_kind must be'),
                          ((2**40, 2**40, 4), b'too large for one launch')):
        assert lib.wfk_avg_plan_create(*args, C.byref(h)) == -1 and not h, args
        assert message in lib.wfk_last_error(), (args, lib.wfk_last_error())
    assert lib.wfk_avg_plan_create(16, 1, 4, None) == -1
    assert lib.wfk_avg_apply(None, None, 1, 16, 0, None, 16, None, 16, 0, None) == -1
    assert b'null plan' in lib.wfk_last_error()
    assert lib.wfk_avg_plan_destroy(None) == 0
    assert lib.wfk_avg_kernel_name(None, 10, 1) == b'' and lib.wfk_avg_splits(None, 10, 0) == 0


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_avg_plan_create', 'wfk_avg_apply', 'wfk_avg_splits', 'wfk_avg_kernel_name',
                 'wfk_avg_plan_destroy'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_avg_plan wfk_avg_plan;' in src
    assert lib.wfk_abi_version() == 2


def test_average_traces_without_a_device(no_library):
    for shape in ((0, 16), (5, 0), (0, 0)):
        for dtype in (np.int16, np.float32, np.float64):
            mean = average_traces(np.zeros(shape, dtype=dtype), steps=3)
            assert mean.shape == (3, shape[1]) and mean.dtype == np.float64 and np.isnan(mean).all()
            mean, var = average_traces(np.zeros(shape, dtype=dtype), steps=2, return_var=True)
            assert mean.shape == var.shape == (2, shape[1]) and np.isnan(var).all() and var is not mean
    with pytest.raises(ValueError, match='shape'):
        average_traces(np.zeros(16))
    with pytest.raises(ValueError, match='complex'):
        average_traces(np.zeros((2, 4), dtype=complex))
    with pytest.raises(ValueError, match='steps >= 1'):
        average_traces(np.zeros((2, 4)), steps=0)
    with pytest.raises(ValueError, match='fits neither'):
        average_traces(np.zeros((2, 4), dtype=np.longdouble))
    assert utils.__all__[-2:] == ['TraceAverager', 'average_traces']


def test_finish_on_the_host():
    """finish_torch is plain torch: it runs on host tensors as well"""
    av = TraceAverager(2, steps=3)
    total = torch.tensor([[6, -3], [4, 4], [0, 0]], dtype=torch.int64)
    total_sq = torch.tensor([[14, 5], [8, 16], [0, 0]], dtype=torch.int64)
    mean, var = av.finish_torch(total, total_sq, np.array([3, 2, 0]))
    assert mean.dtype == var.dtype == torch.float64
    assert mean[:2].tolist() == [[2.0, -1.0], [2.0, 2.0]] and torch.isnan(mean[2]).all() and torch.isnan(var[2]).all()
    assert np.allclose(var[:2].numpy(), [[14 / 3 - 4, 5 / 3 - 1], [0.0, 4.0]], rtol=0, atol=1e-15)
    assert av.finish_torch(total, None, av.counts(5))[1] is None
