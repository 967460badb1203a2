"""The segment player without a device (distortion.SegmentPlayer / play_rows, _engine.segment_play_arguments,
csrc/wfk_segment_play.hip): the two forms of the referee tests/segment_play_ref.py against each other and against
distortion.expand_segments on random good tables, its report on planted differences, each condition of a bad row by
itself, every refusal that comes before any device work -- Python's and, through ctypes, the library's -- and the
stage's lines of the row rule through a stand-alone host program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import segment_library_ref
import segment_play_ref as ref
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(table, packed, used, n, idle=0, k=1, capacity=None, expect=None):
    """the referee in both forms, held to each other -> (outs, report)"""
    a = ref.play_ref(table, packed, used, n, idle, k, capacity, expect, form='loop')
    b = ref.play_ref(table, packed, used, n, idle, k, capacity, expect, form='searchsorted')
    assert np.array_equal(a[1], b[1]), (a[1], b[1])
    for x, y in zip(a[0], b[0]):
        assert (x is None and y is None) or (x.dtype == y.dtype == np.int16 and np.array_equal(x, y))
    return a


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('n', [0, 1, 2, 3, 17, 64, 65])
def test_referee_forms_agree_with_each_other_and_with_expand_segments(n, k):
    for idle in ([5], [5, -9][:k]):
        for seed in range(6):
            rows = [ref.random_table(n, k, 10 * seed + i, lead=i, shuffle_offsets=bool(i)) for i in range(3)]
            rows.append(ref.random_table(n, k, seed, dense=True))
            table, packed, used = ref.stack_rows(rows, k, max_segments=max(len(r[0]) for r in rows) + 2)
            outs, report = both(table, packed, used, n, idle, k)
            for r, (t, p, _) in enumerate(rows):
                want = distortion.expand_segments(t, p, n, idle, width=k)
                assert outs[r].dtype == want.dtype and np.array_equal(outs[r], want)
                assert report[r].tolist() == [int(t[:, 1].sum()), 0, 0, -1]
            # the rows themselves as expect: nothing differs; with the library's builder of offsets with gaps and a lead
            _, report = both(table, packed, used, n, idle, k, expect=np.stack(outs).reshape(len(rows), k * n))
            assert report[:, 1:].tolist() == [[0, 0, -1]] * len(rows)
    pieces = segment_library_ref.shapes_of([1 + (3 * d) % 5 for d in range(4)], k, n)
    t, p, kept = segment_library_ref.row_of(pieces, k, gaps=[0, 3, 1], lead=2)   # starts 3 apart past each piece
    n_row = int(t[-1, 0] + t[-1, 1]) + n
    table, packed, used = ref.stack_rows([(t, p, kept)], k)
    outs, report = both(table, packed, used, n_row, [1, 2][:k], k)
    assert np.array_equal(outs[0], distortion.expand_segments(t, p, n_row, [1, 2][:k], width=k))


def planted_case(k):
    """a row of 60 samples with plays [5, 9), [9, 12) (touching), [20, 31), [40, 41): -> (table, packed, used, out)"""
    t = np.array([[5, 4, 3], [9, 3, 20], [20, 11, 8], [40, 1, 0]], dtype=np.int32)
    packed = np.arange(100, 100 + 30 * k).astype(np.int16)
    table, pk, used = ref.stack_rows([(t, packed, 30)], k)
    outs, report = both(table, pk, used, 60, [-1, -2][:k], k)
    assert report.tolist() == [[19, 0, 0, -1]]
    return table, pk, used, outs[0]


@pytest.mark.parametrize('k', [1, 2])
def test_report_of_the_referee_on_planted_differences(k):
    table, packed, used, out = planted_case(k)
    idle = [-1, -2][:k]

    def report(*codes):
        e = out.copy()
        for c in set(codes):
            e[c] ^= 0x10
        return both(table, packed, used, 60, idle, k, expect=e[None])[1][0].tolist()

    assert report() == [19, 0, 0, -1]
    assert report(k * 5) == [19, 1, 0, 5]                                   # the first code of a play
    assert report(k * 31 - 1) == [19, 1, 0, 30]                             # the last code of a play
    assert report(k * 40, k * 41 - 1) == [19, 1, 0, 40]                     # a one-sample play, all its codes: one sample
    assert report(k * 2) == [19, 0, 1, 2]                                   # a stray sample before the first play
    assert report(k * 15) == [19, 0, 1, 15]                                 # in the first gap
    assert report(k * 59 + k - 1) == [19, 0, 1, 59]                         # in the last gap: the row's last code
    assert report(k * 12) == [19, 0, 1, 12] and report(k * 11) == [19, 1, 0, 11]   # either side of a play's end
    assert report(k * 8, k * 9) == [19, 2, 0, 8]                            # either side of the touching edge
    assert report(k * 50, k * 25, k * 33, k * 10) == [19, 2, 2, 10]         # first: the lowest of several
    assert report(k * 25, k * 3, k * 50) == [19, 1, 2, 3]
    if k == 2:
        assert report(2 * 22 + 1) == [19, 1, 0, 22]                         # the second code of a pair only
        assert report(2 * 22 + 1, 2 * 22) == [19, 1, 0, 22]                 # both codes: still one sample
        assert report(2 * 17 + 1) == [19, 0, 1, 17]


@pytest.mark.parametrize('k', [1, 2])
def test_each_condition_of_a_bad_row_by_itself(k):
    n, cap, ms = 60, 30, 5
    t = np.array([[5, 4, 3], [9, 3, 20], [20, 11, 8], [40, 1, 0]], dtype=np.int32)
    packed = np.arange(30 * k).astype(np.int16)

    def verdict(count=4, **entries):
        """the report of the row with table[j] = entry for j, entry in entries"""
        tt = np.full((1, ms, 3), -7, dtype=np.int32)
        tt[0, :4] = t
        for j, e in entries.items():
            tt[0, int(j[1:])] = e
        outs, report = both(tt, packed[None], np.array([[count, 0]], dtype=np.int64), n, 0, k, capacity=cap)
        assert (outs[0] is None) == (report[0, 0] == -1) and (report[0, 0] >= 0 or report[0].tolist() == [-1] * 4)
        return 'bad' if outs[0] is None else 'good'

    assert verdict() == 'good' and verdict(count=0) == 'good'
    assert verdict(count=-1) == 'bad' and verdict(count=ms + 1) == 'bad'
    assert verdict(count=ms) == 'bad'                                       # entry 4 is the filler [-7, -7, -7]
    assert verdict(count=ms, j4=[41, 19, 11]) == 'good'                     # count = max_segments, to the row's end
    assert verdict(j1=[9, 0, 20]) == 'bad' and verdict(j1=[9, -1, 20]) == 'bad'        # length 0, negative
    assert verdict(j0=[-1, 4, 3]) == 'bad' and verdict(j0=[0, 4, 3]) == 'good'         # a negative start
    assert verdict(j3=[40, 21, 0]) == 'bad' and verdict(j3=[40, 20, 0]) == 'good'      # start + length = n + 1, n
    assert verdict(j2=[20, 11, -1]) == 'bad' and verdict(j2=[20, 11, 0]) == 'good'     # a negative offset
    assert verdict(j2=[20, 11, cap - 10]) == 'bad' and verdict(j2=[20, 11, cap - 11]) == 'good'   # capacity + 1
    assert verdict(j1=[9, 11, 0]) == 'good'                                 # touching but ordered, on both sides
    assert verdict(j1=[8, 3, 20]) == 'bad'                                  # overlapping by one sample
    assert verdict(j1=[9, 12, 0]) == 'bad'
    assert verdict(j2=[4, 1, 8]) == 'bad'                                   # disjoint, but not ascending
    assert verdict(j3=[2**31 - 1, 2**31 - 1, 0]) == 'bad'                   # formed in 64 bits
    assert verdict(count=3, j3=[0, 0, -5]) == 'good'                        # beyond count: not looked at


REFUSALS = ((dict(n=-1), 'n must lie in'), (dict(n=2**31), 'n must lie in'), (dict(n=2.5), 'n must be a whole number'),
            (dict(rows=0), 'rows must be at least 1'), (dict(rows=1.5), 'rows must be a whole number'),
            (dict(width=3), 'width must be 1 or 2'), (dict(width=0), 'width must be 1 or 2'),
            (dict(max_segments=-1), 'max_segments must not be negative'),
            (dict(max_segments=2**30 + 1), 'max_segments must not exceed'),
            (dict(capacity=-1), 'capacity must lie in'), (dict(capacity=2**31), 'capacity must lie in'),
            (dict(capacity=2.5), 'capacity must be a whole number'))


def test_arguments_refuse_and_default():
    A = _engine.segment_play_arguments
    for kw, message in REFUSALS:
        with pytest.raises(ValueError, match=message):
            A(**dict(dict(n=100, rows=2, max_segments=8, capacity=64), **kw))
    assert A(100, 2, 1, 8, 64) == (100, 2, 1, 8, 64) and A(0) == (0, 1, 1, 0, 0)
    assert A(np.int64(3), 2.0, np.int32(2), 5.0, 2**31 - 1) == (3, 2, 2, 5, 2**31 - 1)
    assert A(10, capacity=1000) == (10, 1, 1, 0, 1000)                     # a library's room is not bound by n
    I = _engine.segment_play_idle
    assert I(0, 1) == (0, 0) and I(-5, 2) == (-5, -5) and I([3, -4], 2) == (3, -4) and I(np.int16(7), 1) == (7, 7)
    for idle, k, message in (([1, 2], 1, 'one code or one per code'), ([1, 2, 3], 2, 'one code or one per code'),
                             ([], 2, 'one code or one per code'), (1.5, 1, 'idle must be a whole number'),
                             (32768, 1, 'idle must lie in'), ([0, -32769], 2, 'idle must lie in')):
        with pytest.raises(ValueError, match=message):
            I(idle, k)


def test_stage_refuses_and_needs_no_device():
    for kw, message in REFUSALS:
        kw = dict(dict(n=100, batch=2, max_segments=8, capacity=64),
                  **{('batch' if key == 'rows' else key): v for key, v in kw.items()})
        with pytest.raises(ValueError, match='SegmentPlayer: ' + message):
            distortion.SegmentPlayer(**kw)
    st = distortion.SegmentStage(100, batch=3, width=2, align=16)
    player = distortion.SegmentPlayer.of(st)
    assert (player.n, player.batch, player.width, player.max_segments, player.capacity, player.plan) == \
        (100, 3, 2, 4, 100, None)
    assert distortion.SegmentPlayer.of(st, 100).n == 100
    lib = distortion.SegmentLibrary.of(st, lib_capacity=40)
    of_lib = distortion.SegmentPlayer.of(lib, 100)
    assert (of_lib.n, of_lib.batch, of_lib.width, of_lib.max_segments, of_lib.capacity) == (100, 3, 2, 4, 40)
    for args, message in (((st, 99), 'is not the n of the stage'), ((lib,), 'does not know n'),
                          ((lib, -1), 'n must lie in'), ((5,), 'takes a SegmentStage or a SegmentLibrary')):
        with pytest.raises(ValueError, match='SegmentPlayer: .*' + message):
            distortion.SegmentPlayer.of(*args)
    for x in (player, of_lib, lib, st):
        x.close()


def test_wrapper_refuses_before_any_device_work():
    P = distortion.play_rows
    t, p = np.zeros((2, 3), dtype=np.int32), np.zeros(8, dtype=np.int16)
    for args, kw, message in ((([(t, p)], 10), dict(width=3), 'width must be 1 or 2'), (([], 10), {}, 'no rows'),
                              (([(t.astype(np.int64), p)], 10), {}, r'row 0: the table must be \(count, 3\) int32'),
                              (([(t, p), (t[:, :2], p)], 10), {}, 'row 1: the table must be'),
                              (([(t, p.astype(np.int32))], 10), {}, 'row 0: the packed codes must be 1-D int16'),
                              (([(t, p[:7])], 10), dict(width=2), 'row 0: the packed codes must be'),
                              (([(t, p), 5], 10), {}, 'list of'),
                              (([(t, p)], -1), {}, 'n must lie in'), (([(t, p)], 2**31), {}, 'n must lie in'),
                              (([(t, p)], 1.5), {}, 'n must be a whole number'),
                              (([(t, p)], 10), dict(idle=[1, 2]), 'idle is one code or one per code'),
                              (([(t, p)], 10), dict(idle=40000), 'idle must lie in'),
                              (([(t, p)], 10), dict(expect=np.zeros((1, 11), np.int16)), r'expect must be .*\(1, 10\)'),
                              (([(t, p)], 10), dict(expect=np.zeros((1, 10), np.int32)), 'expect must be an int16'),
                              (([(t, p)], 10), dict(expect=np.zeros((1, 10), np.int16), width=2),
                               r'expect must be .*\(1, 20\)')):
        with pytest.raises(ValueError, match='play_rows: .*' + message):
            P(*args, **kw)


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_segment_play_plan_create', 'wfk_segment_play_apply', 'wfk_segment_play_kernel_name',
                 'wfk_segment_play_plan_destroy', 'wfk_segment_play_span'):
        assert name + '(' in src and hasattr(lib, name)
    assert 'wfk_segment_play_apply() enqueues its two kernels' in src
    assert src.count('ONE STREAM AT A TIME') >= 3 and 'BY VALUE per apply' in src and 'NARROWER than expand_segments' in src
    assert '#define WFK_ABI_VERSION 2 ' in src and lib.wfk_abi_version() == 2
    rule = open(os.path.join(ROOT, 'waveforms_amd', 'csrc', 'wfk_row_rule.h')).read()
    assert 'int wfk_segment_play_row_rule(' in rule
    assert 'NARROWER than `expand_segments`' in distortion.SegmentPlayer.__doc__


def test_library_refuses_before_it_looks_for_a_device():
    lib = _engine.lib()
    h = C.c_void_p()
    for args, message in (((-1, 2, 1, 4, 4), b'n must lie in [0, 2^31 - 1]'), ((2**31, 2, 1, 4, 4), b'n must lie in'),
                          ((10, 0, 1, 4, 4), b'rows must be at least 1'), ((10, 2, 3, 4, 4), b'width must be 1 or 2'),
                          ((10, 2, 0, 4, 4), b'width must be 1 or 2'),
                          ((10, 2, 1, -1, 4), b'max_segments must not be negative'),
                          ((10, 2, 1, 2**30 + 1, 4), b'max_segments must not exceed 2^30'),
                          ((10, 2, 1, 4, -1), b'capacity must lie in [0, 2^31 - 1]'),
                          ((10, 2, 1, 4, 2**31), b'capacity must lie in [0, 2^31 - 1]'),
                          ((2**31 - 1, 2**31 - 1, 1, 4, 4), b'too large for one launch')):
        assert lib.wfk_segment_play_plan_create(*args, C.byref(h)) == -1 and not h
        err = lib.wfk_last_error()
        assert err.startswith(b'segment play plan: ') and message in err, err
    assert lib.wfk_segment_play_plan_create(10, 2, 1, 4, 4, None) == -1
    assert lib.wfk_segment_play_apply(None, None, 0, None, 0, None, 0, 0, None, 0, None, 0, None, None) == -1
    assert lib.wfk_segment_play_kernel_name(None, 0) == b'' and lib.wfk_segment_play_span(None) == 0
    assert lib.wfk_segment_play_plan_destroy(None) == 0


BUILDS = {'plain': ['-O3'],
          'sanitized': ['-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan']}


@pytest.mark.parametrize('build', list(BUILDS))
def test_the_row_rule_holds_the_stage_to_its_lines(build, tmp_path):
    exe = tmp_path / f'segment_play_row_rule_{build}'
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', *BUILDS[build],
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'waveforms_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'segment_play_row_rule_host.cpp'), '-o', str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == 'segment play row rule ok' and not r.stderr, (r.stdout, r.stderr)
