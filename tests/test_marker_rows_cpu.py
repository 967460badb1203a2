"""The marker stage (distortion.MarkerStage / marker_rows), everything up to the point a device is needed: the
referee's own properties (tests/marker_rows_ref.py: the brute-force form against the cumulative-sum form, clipping, gap
closing, pulses, special values, pairs, the bit merge), the argument checks that come before any device work, and the
declarations of the header.  Everything is an integer: every comparison is exact."""
import os
import re

import numpy as np
import pytest

import marker_rows_ref as ref
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spikes(n, positions, dtype=np.float64):
    x = np.zeros((1, n), dtype=dtype)
    x[0, list(positions)] = 1.0
    return x


def test_referee_forms_agree_on_random_rows():
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 17):
        for lead in (0, 1, 2, 5):
            for trail in (0, 1, 2, 5):
                for density in (0.1, 0.5):
                    x = (rng.uniform(size=(4, n)) < density) * rng.uniform(-2, 2, (4, n))
                    for group in (1, 2):
                        a, ca = ref.marker_brute(x, lead, trail, 0.0, group)
                        b, cb = ref.marker_cumsum(x, lead, trail, 0.0, group)
                        assert a.dtype == b.dtype == np.uint8 and ca.dtype == cb.dtype == np.int64
                        assert a.shape == b.shape == (4 // group, n) and ca.shape == cb.shape == (4 // group, 2)
                        assert np.array_equal(a, b) and np.array_equal(ca, cb), (n, lead, trail, group)
    for kind in ref.KINDS:                                      # and on every kind of row the builder makes
        x = ref.rows_pattern(4, 257, 5, kind, threshold=0.25, positions=[0, 100, 256])
        lead, trail = [0, 3, 70, 300], [2, 0, 64, 300]
        a, ca = ref.marker_brute(x, lead, trail, 0.25)
        b, cb = ref.marker_ref(x, lead, trail, 0.25)
        assert np.array_equal(a, b) and np.array_equal(ca, cb), kind


def test_referee_clips_the_window_at_the_row_ends():
    m, c = ref.marker_ref(spikes(10, [0]), 3, 2)
    assert m.tolist() == [[1, 1, 1, 0, 0, 0, 0, 0, 0, 0]] and c.tolist() == [[3, 1]]
    m, c = ref.marker_ref(spikes(10, [9]), 3, 2)
    assert m.tolist() == [[0, 0, 0, 0, 0, 0, 1, 1, 1, 1]] and c.tolist() == [[4, 1]]
    m, c = ref.marker_ref(spikes(10, [4]), 4096, 4096)          # windows longer than the row
    assert m.tolist() == [[1] * 10] and c.tolist() == [[10, 1]]
    m, c = ref.marker_ref(spikes(10, [4]), 2, 1)
    assert m.tolist() == [[0, 0, 1, 1, 1, 1, 0, 0, 0, 0]] and c.tolist() == [[4, 1]]
    m, c = ref.marker_ref(np.zeros((2, 0)), 2, 1)
    assert m.shape == (2, 0) and c.tolist() == [[0, 0], [0, 0]]


def test_referee_closes_gaps_up_to_lead_plus_trail():
    for lead, trail in ((0, 0), (2, 3), (5, 0), (0, 5), (64, 65)):
        for gap, pulses in ((lead + trail, 1), (lead + trail + 1, 2)):
            n = 2 * (lead + trail) + gap + 12
            first = lead + 3
            x = spikes(n, [first, first + gap + 1])             # `gap` inactive samples between the two
            m, c = ref.marker_ref(x, lead, trail)
            assert c[0, 1] == pulses, (lead, trail, gap)
            assert c[0, 0] == 2 * (lead + trail + 1) - max(0, lead + trail - gap)
            assert m[0, first - lead - 1] == 0 and m[0, first - lead] == 1
            assert m[0, first + gap + 1 + trail] == 1 and m[0, first + gap + 2 + trail] == 0


def test_referee_counts_a_marker_that_starts_at_the_first_sample():
    m, c = ref.marker_ref(spikes(8, [0, 1, 5]), 0, 0)
    assert m.tolist() == [[1, 1, 0, 0, 0, 1, 0, 0]] and c.tolist() == [[3, 2]]
    m, c = ref.marker_ref(spikes(8, [2]), 5, 0)
    assert m.tolist() == [[1, 1, 1, 0, 0, 0, 0, 0]] and c.tolist() == [[3, 1]]
    assert ref.marker_ref(np.ones((1, 8)), 0, 0)[1].tolist() == [[8, 1]]
    assert ref.marker_ref(np.zeros((1, 8)), 9, 9)[1].tolist() == [[0, 0]]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_referee_special_values(dtype):
    for threshold in (0.0, 0.25, 0.1):
        vals, active = ref.specials(threshold, dtype)
        m, _ = ref.marker_ref(vals[None, :], 0, 0, threshold)
        assert np.array_equal(m[0].astype(bool), active)
        names = ['nan', 'inf', 'zero', 'subnormal', 'threshold', 'above']
        want = dict(nan=False, inf=True, zero=False, subnormal=threshold == 0.0, above=True,
                    threshold=float(vals[4]) > threshold)        # float32(0.1) lies above the double 0.1
        for sign in (0, 6):
            for i, name in enumerate(names):
                assert active[sign + i] == want[name], (threshold, name, sign)
    assert np.signbit(ref.specials(0.0)[0][8]) and ref.specials(0.0)[0][8] == 0            # -0.0 is among them
    assert not ref.marker_ref(np.array([[-0.0, 0.0, np.nan, -np.nan]]), 0, 0)[0].any()
    assert ref.marker_ref(np.array([[0.5, np.nextafter(0.5, 1), -0.5, -np.inf]]), 0, 0, 0.5)[0].tolist() == [[0, 1, 0, 1]]


def test_referee_pair_is_the_or_of_its_rows():
    x = ref.rows_pattern(6, 300, 3, 'bursts', burst=5, gap=40)
    one, _ = ref.marker_ref(x, 0, 0)
    two, c2 = ref.marker_ref(x, 0, 0, group=2)
    assert two.shape == (3, 300) and c2.shape == (3, 2)
    for g in range(3):
        assert np.array_equal(two[g], one[2 * g] | one[2 * g + 1])
    assert np.any(two[0] != one[0]) and np.any(two[0] != one[1])
    wide, _ = ref.marker_ref(x, [3, 0, 7], [1, 2, 0], group=2)  # one lead / trail per MARKER row
    for g, (lead, trail) in enumerate(((3, 1), (0, 2), (7, 0))):
        assert np.array_equal(wide[g], ref.marker_brute(x[2 * g:2 * g + 2], lead, trail, 0.0, 2)[0][0])


def test_into_codes_changes_one_bit_and_clears_it_where_the_marker_is_low():
    rng = np.random.default_rng(4)
    m = (rng.uniform(size=(3, 50)) < 0.5).astype(np.uint8)
    for group in (1, 2):
        codes = rng.integers(-32768, 32768, (3, group * 50)).astype(np.int16)
        for bit in (0, 1, 7, 15):
            out = ref.into_codes(codes, m, group, bit)
            assert out.dtype == np.int16 and out.shape == codes.shape
            changed = out.view(np.uint16) ^ codes.view(np.uint16)
            assert not np.any(changed & ~np.uint16(1 << bit))
            assert np.array_equal((out.view(np.uint16) >> bit) & 1, np.repeat(m, group, axis=1))
            was_set = (codes.view(np.uint16) >> bit) & 1
            assert np.any((was_set == 1) & (np.repeat(m, group, axis=1) == 0))          # some bits do get cleared
            assert np.array_equal(ref.into_codes(out, m, group, bit), out)              # a second merge: the same
    assert ref.into_codes(np.array([[-1, -1]], dtype=np.int16), np.array([[0]]), 2, 15).tolist() == [[32767, 32767]]


REFUSALS = [                                                   # (keywords of MarkerStage(64, ...), message)
    (dict(threshold=[0.0, 0.0, 0.0, -1.0]), 'row 3: threshold is negative'),
    (dict(threshold=[0.0, np.nan]), 'row 1: threshold is not finite'),
    (dict(threshold=[np.inf]), 'row 0: threshold is not finite'),
    (dict(lead=[0, 0, 0, 4097]), 'row 3: lead exceeds 4096'),
    (dict(lead=[-1, 0]), 'row 0: lead is negative'),
    (dict(trail=[0, -1]), 'row 1: trail is negative'),
    (dict(trail=[0, 0, 5000]), 'row 2: trail exceeds 4096'),
    (dict(lead=[1.5]), 'lead is a number of samples'),
    (dict(lead=[1], group=3), 'group must be 1 or 2'),
    (dict(lead=[1], group=0), 'group must be 1 or 2'),
    (dict(batch=3, group=2), '3 rows are no multiple of the group'),
    (dict(lead=[1], dtype=np.int16), 'dtype must be float64 or float32'),
]


def test_stage_refuses_before_any_device_work():
    for kw, message in REFUSALS:
        with pytest.raises(ValueError, match=message):
            distortion.MarkerStage(64, **kw)
    with pytest.raises(ValueError, match='batch'):
        distortion.MarkerStage(64, lead=3, trail=2)                                  # scalars need batch=
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.MarkerStage(64, lead=[1, 2, 3], batch=4, group=2)
    with pytest.raises(ValueError, match='for 3 rows'):
        distortion.MarkerStage(64, lead=[1, 2, 3], trail=[1, 2])
    with pytest.raises(ValueError, match='no rows'):
        distortion.MarkerStage(64, batch=0)
    with pytest.raises(ValueError, match='no rows'):
        distortion.MarkerStage(64, lead=[])
    with pytest.raises(ValueError, match='n >= 0'):
        distortion.MarkerStage(-1, batch=2)
    with pytest.raises(NotImplementedError):
        distortion.MarkerStage(64, batch=2, dtype=np.complex128)


def test_plan_refuses_before_any_device_work():
    P = _engine.MarkerRowsPlan
    for args, message in ((([0.0, -1.0], [0, 0], [0, 0], 64), 'row 1: threshold is negative'),
                          (([0.0, np.inf], [0, 0], [0, 0], 64), 'row 1: threshold is not finite'),
                          (([0.0], [4097], [0], 64), 'row 0: lead exceeds 4096'),
                          (([0.0], [-1], [0], 64), 'row 0: lead is negative'),
                          (([0.0], [0], [-2], 64), 'row 0: trail is negative'),
                          (([0.0], [0], [4097], 64), 'row 0: trail exceeds 4096'),
                          (([0.0], [0], [0], 64, 3), 'group must be 1 or 2'),
                          (([0.0], [0], [0], -1), 'n >= 0'),
                          (([0.0], [0, 1], [0], 64), 'one of each'),
                          (([], [], [], 64), 'at least one row'),
                          (([0.0], [0], [0], 64, 1, np.int32), 'dtype must be float64 or float32')):
        with pytest.raises(ValueError, match=message):
            P(*args)
    with pytest.raises(NotImplementedError):
        P([0.0], [0], [0], 64, 1, np.complex64)
    th, le, tr, n, group, dtype = _engine.marker_rows_arguments([0.5, 0], [4096, 0], [0, 7], 10, 2, np.float32)
    assert th.dtype == np.float64 and le.dtype == tr.dtype == np.int32 and le.tolist() == [4096, 0]
    assert (n, group, dtype) == (10, 2, np.dtype(np.float32)) and _engine.MARKER_MAX_EDGE == 4096


def test_wrapper_refuses_before_any_device_work():
    sig = np.zeros((4, 16))
    for kw, message in REFUSALS:
        if 'batch' in kw or 'dtype' in kw:
            continue
        rows = max([np.size(v) for v in kw.values() if np.ndim(v) > 0] + [1]) * (2 if kw.get('group') == 2 else 1)
        with pytest.raises(ValueError, match=message):
            distortion.marker_rows(np.zeros((rows, 16)), **kw)
    with pytest.raises(ValueError, match='3 rows are no multiple of the group'):
        distortion.marker_rows(np.zeros((3, 16)), group=2)
    with pytest.raises(ValueError, match='2-D'):
        distortion.marker_rows(np.zeros(16))
    with pytest.raises(ValueError, match='2-D'):
        distortion.marker_rows(np.zeros((2, 2, 4)))
    with pytest.raises(ValueError, match='for 4 rows'):
        distortion.marker_rows(sig, lead=[1, 2])
    with pytest.raises(ValueError, match='for 2 rows'):
        distortion.marker_rows(sig, trail=[1, 2, 3, 4], group=2)
    with pytest.raises(ValueError, match='no rows'):
        distortion.marker_rows(np.zeros((0, 16)))
    for bit in (-1, 16):
        with pytest.raises(ValueError, match='bit must lie in'):
            distortion.marker_rows(sig, codes=np.zeros((4, 16), dtype=np.int16), bit=bit)
    for bad in (np.zeros((4, 16), dtype=np.int32), np.zeros((4, 32), dtype=np.int16), np.zeros((2, 16), dtype=np.int16)):
        with pytest.raises(ValueError, match='codes must be int16'):
            distortion.marker_rows(sig, codes=bad)
    with pytest.raises(NotImplementedError):
        distortion.marker_rows(sig + 0j)


def test_wrapper_handles_empty_rows_without_a_device():
    m = distortion.marker_rows(np.zeros((2, 0)), lead=3, trail=[1, 2])
    assert m.shape == (2, 0) and m.dtype == np.uint8
    m, counts = distortion.marker_rows(np.zeros((2, 0), dtype=np.float32), group=2, return_counts=True)
    assert m.shape == (1, 0) and m.dtype == np.uint8
    assert counts.shape == (1, 2) and counts.dtype == np.int64 and not counts.any()
    codes = distortion.marker_rows(np.zeros((2, 0)), group=2, codes=np.zeros((1, 0), dtype=np.int16), bit=3)
    assert codes.shape == (1, 0) and codes.dtype == np.int16
    with pytest.raises(ValueError, match='row 0: lead exceeds 4096'):
        distortion.marker_rows(np.zeros((2, 0)), lead=5000)


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_marker_rows_plan_create', 'wfk_marker_rows_apply', 'wfk_marker_rows_apply_codes',
                 'wfk_marker_rows_span', 'wfk_marker_rows_kernel_name', 'wfk_marker_rows_plan_destroy'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_marker_rows_plan wfk_marker_rows_plan;' in src
    assert re.search(r'^#define WFK_MARKER_MAX_EDGE 4096\b', src, re.M)
    assert lib.wfk_abi_version() == 2


def test_library_refuses_before_any_device_work():
    """the C side's own refusals come before it looks for a device: WFK_EINVAL (-1) here, with the row named"""
    import ctypes as C
    lib = _engine.lib()
    h = C.c_void_p()
    create = lib.wfk_marker_rows_plan_create

    def refused(n, batch, kind, group, thr, lead, trail):
        rows = len(thr)
        rc = create(n, batch, kind, group, (C.c_double * rows)(*thr), (C.c_int32 * rows)(*lead),
                    (C.c_int32 * rows)(*trail), C.byref(h))
        assert rc == -1 and not h, (n, batch, kind, group, thr, lead, trail, rc)
        return lib.wfk_last_error()

    z4 = [0] * 4
    assert b'row 3: threshold is negative' in refused(64, 4, 0, 1, [0.0, 0.0, 0.0, -0.5], z4, z4)
    assert b'row 3: threshold is not finite' in refused(64, 4, 0, 1, [0.0, 0.0, 0.0, float('nan')], z4, z4)
    assert b'row 1: threshold is not finite' in refused(64, 4, 1, 2, [0.0, float('inf')], [0, 0], [0, 0])
    assert b'row 3: lead exceeds 4096' in refused(64, 4, 0, 1, [0.0] * 4, [0, 0, 0, 4097], z4)
    assert b'row 0: lead is negative' in refused(64, 4, 0, 1, [0.0] * 4, [-1, 0, 0, 0], z4)
    assert b'row 2: trail is negative' in refused(64, 4, 0, 1, [0.0] * 4, z4, [0, 0, -1, 0])
    assert b'row 1: trail exceeds 4096' in refused(64, 4, 0, 1, [0.0] * 4, z4, [0, 4097, 0, 0])
    assert b'group must be 1 or 2' in refused(64, 4, 0, 3, [0.0] * 4, z4, z4)
    assert b'group must be 1 or 2' in refused(64, 4, 0, 0, [0.0] * 4, z4, z4)
    assert b'3 rows are no multiple of the group' in refused(64, 3, 0, 2, [0.0] * 4, z4, z4)
    assert b'n must not be negative' in refused(-1, 4, 0, 1, [0.0] * 4, z4, z4)
    assert b'kind must be F64 or F32' in refused(64, 4, 2, 1, [0.0] * 4, z4, z4)
    refused(64, 0, 0, 1, [0.0] * 4, z4, z4)
    for n, group in ((2**62, 1), (2**62, 2), (2**46, 1)):                               # more than 2^31 - 1 workgroups
        assert b'too large for one launch' in refused(n, 4, 0, group, [0.0] * 4, z4, z4)
    assert create(64, 4, 0, 1, None, None, None, C.byref(h)) == -1 and not h
    assert lib.wfk_marker_rows_apply(None, None, 64, None, 64, None, None) == -1
    assert lib.wfk_marker_rows_apply_codes(None, None, 64, None, 64, 0, None, None) == -1
    assert lib.wfk_marker_rows_plan_destroy(None) == 0
    assert lib.wfk_marker_rows_kernel_name(None, 0, 0) == b''
    assert lib.wfk_marker_rows_kernel_name(None, 1, 1) == b''
    assert lib.wfk_marker_rows_span(None, 0) == 0
