"""The segment library without a device (distortion.SegmentLibrary / library_rows, _engine.segment_library_arguments,
csrc/wfk_segment_library.hip): the two forms of the referee tests/segment_library_ref.py against each other and against
cases worked out by hand, the round trip through expand_segments, every refusal that comes before any device work --
Python's and, through ctypes, the library's -- and the stage's lines of the row rule through a stand-alone host
program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import segment_library_ref as ref
import segment_rows_ref
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(table, packed, used, k=1, capacity=None):
    """the referee in both forms, held to each other -> (plays, slots, library, lib_used)"""
    a = ref.library_ref(table, packed, used, k, capacity, form='dict')
    b = ref.library_ref(table, packed, used, k, capacity, form='loop')
    assert np.array_equal(a[3], b[3])
    for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]):
        assert (x is None and y is None) or (x.dtype == y.dtype and np.array_equal(x, y))
    return a


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('c', [0, 1, 2, 5, 64, 65])
def test_referee_forms_agree_on_random_rows(c, k):
    for D in sorted({1, 2, max(c, 1)}):
        shapes = ref.shapes_of([1 + (3 * d) % 11 for d in range(D)], k, 100 * c + D)
        rows = [ref.drawn_row(c, shapes, k, seed, gaps=gaps) for seed, gaps in ((1, None), (2, [0, 3, 1]))]
        table, packed, used = ref.stack_rows(rows, k, max_segments=c + 2)
        plays, slots, library, lib_used = both(table, packed, used, k)
        for r, (t, _, _, draw) in enumerate(rows):
            assert lib_used[r, 0] == len(set(draw.tolist())) and len(plays[r]) == c
            assert np.array_equal(plays[r][:, :2], t[:, :2])
            order = list(dict.fromkeys(draw.tolist()))                  # the shapes in order of first occurrence
            assert slots[r].tolist() == [order.index(d) for d in draw.tolist()]
            assert np.array_equal(library[r], np.concatenate([shapes[d] for d in order]) if order else library[r][:0])
            assert lib_used[r, 1] == sum(len(shapes[d]) // k for d in order)


def test_referee_by_hand():
    a, b = np.array([5, 6, 7], dtype=np.int16), np.array([5, 6], dtype=np.int16)
    t, p, kept = ref.row_of([a, b, a, b, a[:1]], 1)                     # b is a prefix of a; a[:1] of both
    table, packed, used = ref.stack_rows([(t, p, kept)], 1)
    plays, slots, library, lib_used = both(table, packed, used)
    assert slots[0].tolist() == [0, 1, 0, 1, 2] and lib_used.tolist() == [[3, 6]]
    assert plays[0][:, 2].tolist() == [0, 3, 0, 3, 5] and library[0].tolist() == [5, 6, 7, 5, 6, 5]
    assert plays[0][:, :2].tolist() == t[:, :2].tolist()
    pair = np.array([1, 2, 3, 4], dtype=np.int16)                       # k = 2: two samples
    t, p, kept = ref.row_of([pair, ref.variant(pair, -1), pair], 2)
    plays, slots, library, lib_used = both(*ref.stack_rows([(t, p, kept)], 2), k=2)
    assert slots[0].tolist() == [0, 1, 0] and lib_used.tolist() == [[2, 4]] and plays[0][:, 2].tolist() == [0, 2, 0]
    assert library[0].tolist() == [1, 2, 3, 4, 1, 2, 3, 5]
    plays, slots, library, lib_used = both(np.zeros((1, 0, 3), np.int32), np.zeros((1, 0), np.int16),
                                           np.zeros((1, 2), np.int64))
    assert lib_used.tolist() == [[0, 0]] and plays[0].shape == (0, 3) and len(library[0]) == 0


def test_referee_marks_the_rows_that_cannot_be_read():
    shapes = ref.shapes_of([4, 4], 1, 3)
    good = ref.drawn_row(3, shapes, 1, 4)
    table, packed, used = ref.stack_rows([good] * 10, 1, max_segments=4, capacity=12)
    cap = 12
    used[1, 0] = 5                                                      # count = max_segments + 1
    used[2, 1] = cap + 1
    used[3, 0] = -1
    used[4, 1] = -1
    table[5, 1, 1] = 0
    table[6, 2, 1] = -1
    table[7, 0, 2] = -1
    table[8, 2] = [0, 5, cap - 4]                                       # offset + length = capacity + 1
    table[9, 1, 1:] = 2**31 - 1
    _, _, library, lib_used = both(table, packed, used, capacity=cap)
    assert lib_used[0].tolist() == [len(set(good[3].tolist())), 4 * len(set(good[3].tolist()))]
    assert np.all(lib_used[1:] == -1) and all(y is None for y in library[1:])
    table[8, 2] = [0, 4, cap - 4]                                       # ... = capacity: good
    table[5, 1, 1] = 1
    table[5, 3] = [0, 0, -5]                                            # beyond count: not looked at
    assert both(table, packed, used, capacity=cap)[3][[5, 8], 0].min() > 0


@pytest.mark.parametrize('k', [1, 2])
def test_expand_segments_of_the_library_equals_that_of_the_packed_codes(k):
    n = 3000
    m = segment_rows_ref.bursts_mask(3, n, 21, duty=0.1, gate=8)
    codes = np.where(np.repeat(m, k, axis=1), np.int16(7), np.int16(0)).astype(np.int16)   # equal pulses repeat
    tables, packed, used = segment_rows_ref.segment_ref(codes, k, 4, bit=0)
    ms, cap = int(used[:, 0].max()), int(used[:, 1].max())
    table, pk, u = ref.stack_rows([(tables[r], packed[r], int(used[r, 1])) for r in range(3)], k, ms, cap)
    plays, slots, library, lib_used = both(table, pk, u, k)
    for r in range(3):
        back = distortion.expand_segments(plays[r], library[r], n, 0, width=k)
        assert np.array_equal(back, distortion.expand_segments(tables[r], packed[r], n, 0, width=k))
        assert np.array_equal(back, codes[r]) and lib_used[r, 0] < used[r, 0] and lib_used[r, 1] < used[r, 1]
    P, S, Y, lu = ref.expected_outputs(table, pk, u, k, 5, (-1, -2, -3))                    # the cut is by position
    assert np.array_equal(lu, lib_used) and np.array_equal(Y[0], library[0][:5 * k])
    assert np.array_equal(P[0, :len(plays[0])], plays[0]) and np.all(P[0, len(plays[0]):] == -1)


REFUSALS = ((dict(rows=0), 'rows must be at least 1'), (dict(rows=1.5), 'rows must be a whole number'),
            (dict(width=3), 'width must be 1 or 2'), (dict(width=0), 'width must be 1 or 2'),
            (dict(max_segments=-1), 'max_segments must not be negative'),
            (dict(max_segments=2**30 + 1), 'max_segments must not exceed'),
            (dict(capacity=-1), 'capacity must lie in'), (dict(capacity=2**31), 'capacity must lie in'),
            (dict(lib_capacity=-1), 'lib_capacity must lie in'), (dict(lib_capacity=65), 'lib_capacity must lie in'),
            (dict(lib_capacity=2.5), 'lib_capacity must be a whole number'))


def test_arguments_refuse_and_default():
    A = _engine.segment_library_arguments
    for kw, message in REFUSALS:
        with pytest.raises(ValueError, match=message):
            A(**dict(dict(rows=2, max_segments=8, capacity=64), **kw))
    assert A(2, 1, 8, 64) == (2, 1, 8, 64, 64) and A(2, 2, 8, 64, 10) == (2, 2, 8, 64, 10)
    assert A() == (1, 1, 0, 0, 0) and A(np.int64(3), 2.0, np.int32(4), 5.0, 0) == (3, 2, 4, 5, 0)


def test_stage_refuses_and_needs_no_device():
    for kw, message in REFUSALS:
        kw = dict(dict(batch=2, max_segments=8, capacity=64),
                  **{('batch' if key == 'rows' else key): v for key, v in kw.items()})
        with pytest.raises(ValueError, match='SegmentLibrary: ' + message):
            distortion.SegmentLibrary(**kw)
    st = distortion.SegmentStage(100, batch=3, width=2, align=16)
    lib = distortion.SegmentLibrary.of(st)
    assert (lib.batch, lib.max_segments, lib.capacity, lib.width, lib.lib_capacity, lib.plan) == (3, 4, 100, 2, 100, None)
    assert distortion.SegmentLibrary.of(st, lib_capacity=7).lib_capacity == 7
    lib.close()
    st.close()


def test_wrapper_refuses_before_any_device_work():
    L = distortion.library_rows
    t, p = np.zeros((2, 3), dtype=np.int32), np.zeros(8, dtype=np.int16)
    for args, kw, message in ((([(t, p)],), dict(width=3), 'width must be 1 or 2'), (([],), {}, 'no rows'),
                              (([(t.astype(np.int64), p)],), {}, r'row 0: the table must be \(count, 3\) int32'),
                              (([(t, p), (t[:, :2], p)],), {}, 'row 1: the table must be'),
                              (([(t, p.astype(np.int32))],), {}, 'row 0: the packed codes must be 1-D int16'),
                              (([(t, p[:7])],), dict(width=2), 'row 0: the packed codes must be'),
                              (([(t, p), 5],), {}, 'list of')):
        with pytest.raises(ValueError, match='library_rows: .*' + message):
            L(*args, **kw)
    out = L([(t[:0], p[:0]), (t[:0], p)])                                # rows of no segments: no device
    assert len(out) == 2 and out[0][0].shape == (0, 3) and out[0][0].dtype == np.int32
    assert out[1][1].dtype == np.int32 and out[1][2].dtype == np.int16 and len(out[1][2]) == 0


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_segment_library_plan_create', 'wfk_segment_library_apply', 'wfk_segment_library_kernel_name',
                 'wfk_segment_library_plan_destroy'):
        assert name + '(' in src and hasattr(lib, name)
    assert 'wfk_segment_library_apply() enqueues its four kernels' in src
    assert src.count('ONE STREAM AT A TIME') >= 2 and 'WFK_SEGLIB_HASH_BITS' in src
    assert '#define WFK_ABI_VERSION 2 ' in src and lib.wfk_abi_version() == 2


def test_library_refuses_before_it_looks_for_a_device():
    lib = _engine.lib()
    h = C.c_void_p()
    for args, message in (((0, 1, 4, 4, 4), b'rows must be at least 1'), ((2, 3, 4, 4, 4), b'width must be 1 or 2'),
                          ((2, 0, 4, 4, 4), b'width must be 1 or 2'),
                          ((2, 1, -1, 4, 4), b'max_segments must not be negative'),
                          ((2, 1, 2**30 + 1, 4, 4), b'max_segments must not exceed 2^30'),
                          ((2, 1, 4, -1, 0), b'capacity must lie in [0, 2^31 - 1]'),
                          ((2, 1, 4, 2**31, 0), b'capacity must lie in [0, 2^31 - 1]'),
                          ((2, 1, 4, 4, -1), b'lib_capacity must lie in [0, capacity]'),
                          ((2, 1, 4, 4, 5), b'lib_capacity must lie in [0, capacity]'),
                          ((2**31 - 1, 1, 2**30, 4, 4), b'too large for one launch')):
        assert lib.wfk_segment_library_plan_create(*args, C.byref(h)) == -1 and not h
        err = lib.wfk_last_error()
        assert err.startswith(b'segment library plan: ') and message in err, err
    assert lib.wfk_segment_library_plan_create(2, 1, 4, 4, 4, None) == -1
    assert lib.wfk_segment_library_apply(None, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, None) == -1
    assert lib.wfk_segment_library_kernel_name(None, 0) == b''
    assert lib.wfk_segment_library_plan_destroy(None) == 0


BUILDS = {'plain': ['-O3'],
          'sanitized': ['-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan']}


@pytest.mark.parametrize('build', list(BUILDS))
def test_the_row_rule_holds_the_stage_to_its_lines(build, tmp_path):
    exe = tmp_path / f'segment_library_row_rule_{build}'
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', *BUILDS[build],
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'waveforms_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'segment_library_row_rule_host.cpp'), '-o', str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == 'segment library row rule ok' and not r.stderr, (r.stdout, r.stderr)
