"""The segment stage without a device (distortion.SegmentStage / segment_rows / expand_segments,
_engine.segment_rows_arguments, csrc/wfk_segment_rows.hip): the two forms of the referee tests/segment_rows_ref.py
against each other and against cases worked out by hand, the round trip through expand_segments, the tie to the marker
stage's counts, every refusal that comes before any device work -- Python's and, through ctypes, the library's -- and
the stage's lines of the row rule through a stand-alone host program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import marker_rows_ref
import segment_rows_ref as ref
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(codes, width=1, align=1, bit=None, marks=None):
    """the referee in both forms, held to each other -> (tables, packed, used)"""
    a = ref.segment_ref(codes, width, align, bit, marks, form='loop')
    b = ref.segment_ref(codes, width, align, bit, marks, form='vector')
    assert np.array_equal(a[2], b[2])
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    return b


def one_row(mask, align=1, width=1, bit=0, seed=0, **kw):
    m = np.asarray(mask, dtype=bool)[None, :]
    codes = ref.codes_with(m, width, bit, seed, **kw)
    tables, packed, used = both(codes, width, align, bit=bit)
    return codes[0], tables[0].tolist(), packed[0], used[0].tolist()


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('align', [1, 2, 8, 64])
def test_referee_forms_agree_on_random_masks(align, k):
    rng = np.random.default_rng(10 * align + k)
    for n in (0, 1, 2, 3, 17, 64, 65):
        for density in (0.0, 0.05, 0.5, 1.0):
            m = rng.uniform(size=(3, n)) < density
            codes = ref.codes_with(m, k, 3, n, one_code_only=True)
            tables, packed, used = both(codes, k, align, bit=3)
            marks = m.astype(np.uint8) * 7
            t2, p2, u2 = both(ref.codes_with(~m, k, 3, n), k, align, marks=marks)     # the marks form ignores the bit
            assert np.array_equal(used, u2) and all(np.array_equal(a, b) for a, b in zip(tables, t2))
            for g in range(3):
                t = tables[g]
                assert np.all(t[:, 0] % align == 0) and np.all(t[:, 2] % align == 0)
                assert np.all(t[:-1, 1] % align == 0) and np.all(t[:, 1] > 0)
                assert len(t) <= (-(-n // align) + 1) // 2 and used[g, 1] <= n
                assert len(packed[g]) == k * used[g, 1]


def test_referee_all_off_and_all_on():
    for n, align in ((17, 1), (17, 8), (64, 64), (65, 64)):
        _, table, packed, used = one_row(np.zeros(n), align)
        assert table == [] and used == [0, 0] and len(packed) == 0
        codes, table, packed, used = one_row(np.ones(n), align)
        assert table == [[0, n, 0]] and used == [1, n] and np.array_equal(packed, codes)


def test_referee_clips_the_last_partial_granule_to_the_row():
    m = np.zeros(21)
    m[20] = 1                                              # granule 2 of A = 8 holds samples 16 .. 20
    codes, table, packed, used = one_row(m, 8)
    assert table == [[16, 5, 0]] and used == [1, 5] and np.array_equal(packed, codes[16:21])
    m[3] = 1
    codes, table, packed, used = one_row(m, 8)
    assert table == [[0, 8, 0], [16, 5, 8]] and used == [2, 13]


def test_referee_merges_neighbouring_granules_and_keeps_a_gap_of_one():
    m = np.zeros(64)
    m[[7, 8]] = 1                                          # granules 0 and 1
    assert one_row(m, 8)[1] == [[0, 16, 0]]
    m = np.zeros(64)
    m[[7, 16]] = 1                                         # granules 0 and 2: granule 1 is empty
    assert one_row(m, 8)[1] == [[0, 8, 0], [16, 8, 8]]
    m = np.zeros(64)
    m[[0, 2]] = 1
    assert one_row(m, 1)[1] == [[0, 1, 0], [2, 1, 1]] and one_row(m, 2)[1] == [[0, 4, 0]]


def test_referee_a_bit_on_one_code_of_a_pair_counts():
    codes = np.zeros((1, 16), dtype=np.int16)
    codes[0, 5] = 1 << 4                                   # the Q of sample 2
    codes[0, 12] = -32768                                  # bit 15 of the I of sample 6: not bit 4
    tables, packed, used = both(codes, 2, 1, bit=4)
    assert tables[0].tolist() == [[2, 1, 0]] and packed[0].tolist() == [0, 16] and used.tolist() == [[1, 1]]
    tables, _, _ = both(codes, 2, 1, bit=15)
    assert tables[0].tolist() == [[6, 1, 0]]
    tables, _, _ = both(codes, 2, 4, bit=4)
    assert tables[0].tolist() == [[0, 4, 0]]


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('align', [1, 8, 64])
def test_expand_segments_gives_the_codes_back(align, k):
    n, idle = 2000, [-4, 8][:k]
    m = ref.bursts_mask(4, n, 5 + align, duty=0.05, gate=9)                         # gaps of several granules
    codes = ref.codes_with(m, k, 0, 6)
    quiet = np.tile(np.asarray(idle, dtype=np.int16), n)
    codes = np.where(np.repeat(m, k, axis=1), codes, quiet[None, :])                # idle wherever the mask is off
    tables, packed, used = both(codes, k, align, bit=0)
    assert used[:, 0].min() >= 2
    for g in range(4):
        back = distortion.expand_segments(tables[g], packed[g], n, idle if k == 2 else idle[0], width=k)
        assert back.dtype == np.int16 and np.array_equal(back, codes[g])
    noisy = ref.codes_with(m, k, 0, 7)                                              # anything where the mask is off
    tables, packed, _ = both(noisy, k, align, bit=0)
    for g in range(4):
        back = distortion.expand_segments(tables[g], packed[g], n, idle, width=k) if k == 2 else \
            distortion.expand_segments(tables[g], packed[g], n, idle[0])
        on = np.repeat(m[g], k)
        assert np.array_equal(back[on], noisy[g][on])
        kept = np.zeros(n, dtype=bool)
        for s, l, _ in tables[g].tolist():
            kept[s:s + l] = True
        assert np.array_equal(back[~np.repeat(kept, k)], quiet[~np.repeat(kept, k)])
        assert np.all(kept[m[g]])


def test_expand_segments_refuses():
    E = distortion.expand_segments
    p = np.zeros(8, dtype=np.int16)
    for args, message in ((([[0, 4, 0]], p, 8, 0, 3), 'width'), (([[0, 4]], p, 8, 0), 'table'),
                          (([[6, 4, 0]], p, 8, 0), 'segment 0 lies outside the row'),
                          (([[0, 4, 0], [4, 4, 6]], p, 8, 0), 'segment 1 lies outside the packed'),
                          (([[0, 4, 0]], p.astype(np.int32), 8, 0), 'int16'), (([[0, 4, 0]], p, 8, [1, 2]), 'idle')):
        with pytest.raises(ValueError, match=message):
            E(*args)
    assert E(np.zeros((0, 3), dtype=np.int32), p[:0], 3, 5).tolist() == [5, 5, 5]


def test_align_one_counts_what_the_marker_stage_counts():
    x = marker_rows_ref.rows_pattern(6, 300, 11, 'bursts', burst=9, gap=40)
    for k in (1, 2):
        m, counts = marker_rows_ref.marker_ref(x, 3, 2, 0.0, k)
        codes = marker_rows_ref.into_codes(ref.codes_with(np.zeros_like(m), k, 0, 12), m, k, 0)
        _, _, used = both(codes, k, 1, bit=0)
        assert np.array_equal(used[:, 0], counts[:, 1]) and np.array_equal(used[:, 1], counts[:, 0])
        _, _, used = both(codes, k, 1, marks=m)
        assert np.array_equal(used, counts[:, ::-1])


REFUSALS = ((dict(n=-1), 'n must lie in'), (dict(n=2**31), 'n must lie in'), (dict(n=1.5), 'n must be a whole number'),
            (dict(rows=0), 'rows must be at least 1'), (dict(width=3), 'width must be 1 or 2'),
            (dict(width=0), 'width must be 1 or 2'), (dict(align=0), 'align must be a power of two'),
            (dict(align=24), 'align must be a power of two'), (dict(align=8192), 'align must be a power of two'),
            (dict(max_segments=-1), 'max_segments must not be negative'), (dict(capacity=-1), 'capacity must lie in'),
            (dict(capacity=65), 'capacity must lie in'), (dict(capacity=2.5), 'capacity must be a whole number'))


def test_arguments_refuse_and_default():
    A = _engine.segment_rows_arguments
    for kw, message in REFUSALS:
        with pytest.raises(ValueError, match=message):
            A(**dict(dict(n=64, rows=2), **kw))
    assert A(64) == (64, 1, 1, 1, 32, 64)
    assert A(65, 3, 2, 8) == (65, 3, 2, 8, 5, 65)                     # 9 granules: at most 5 segments
    assert A(0, 1, 1, 4096) == (0, 1, 1, 4096, 0, 0)
    assert A(2**31 - 1, 1, 2, 4096, 0, 0)[4:] == (0, 0)
    assert A(np.int64(64), np.int32(2), 1.0, 2.0, 3, 5) == (64, 2, 1, 2, 3, 5)


def test_stage_refuses_and_needs_no_device():
    for kw, message in REFUSALS:
        kw = dict(dict(n=64, batch=2), **{('batch' if key == 'rows' else key): v for key, v in kw.items()})
        with pytest.raises(ValueError, match='SegmentStage: ' + message):
            distortion.SegmentStage(**kw)
    st = distortion.SegmentStage(100, batch=3, width=2, align=16)
    assert (st.n, st.batch, st.width, st.align, st.max_segments, st.capacity, st.plan) == (100, 3, 2, 16, 4, 100, None)
    st.close()


def test_wrapper_refuses_before_any_device_work():
    S = distortion.segment_rows
    codes = np.zeros((2, 64), dtype=np.int16)
    for args, kw, message in (((codes,), {}, 'exactly one'), ((codes,), dict(bit=0, marks=np.zeros((2, 64))), 'exactly one'),
                              ((codes.astype(np.int32),), dict(bit=0), '2-D int16'), ((codes[0],), dict(bit=0), '2-D int16'),
                              ((codes,), dict(bit=16), 'bit must lie'), ((codes,), dict(bit=-1), 'bit must lie'),
                              ((codes,), dict(bit=0, width=3), 'width must be 1 or 2'),
                              ((codes[:, :63],), dict(bit=0, width=2), 'no multiple of the width'),
                              ((codes,), dict(bit=0, align=3), 'align must be a power of two'),
                              ((codes[:0],), dict(bit=0), 'rows must be at least 1'),
                              ((codes,), dict(marks=np.zeros((2, 64)), width=2), r'marks must have the shape \(2, 32\)')):
        with pytest.raises(ValueError, match='segment_rows: .*' + message):
            S(*args, **kw)
    out = S(codes[:, :0], bit=0)                                       # rows of nothing: no device
    assert len(out) == 2 and out[0][0].shape == (0, 3) and out[0][0].dtype == np.int32 and out[0][1].dtype == np.int16


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_segment_rows_plan_create', 'wfk_segment_rows_apply_bit', 'wfk_segment_rows_apply_marks',
                 'wfk_segment_rows_span', 'wfk_segment_rows_kernel_name', 'wfk_segment_rows_plan_destroy'):
        assert name + '(' in src and hasattr(lib, name)
    assert 'wfk_segment_rows_apply_bit() and wfk_segment_rows_apply_marks() enqueue their three kernels' in src
    assert 'ONE STREAM AT A TIME' in src                               # the plan owns the workspace of its launches
    assert '#define WFK_ABI_VERSION 2 ' in src and _engine.SEGMENT_MAX_ALIGN == 4096
    assert '#define WFK_SEGMENT_MAX_ALIGN 4096' in src


def test_library_refuses_before_it_looks_for_a_device():
    lib = _engine.lib()
    h = C.c_void_p()
    for args, message in (((-1, 2, 1, 1, 4, 4), b'n must lie in'), ((2**31, 2, 1, 1, 4, 4), b'n must lie in'),
                          ((64, 0, 1, 1, 4, 4), b'rows must be at least 1'), ((64, 2, 3, 1, 4, 4), b'width must be 1 or 2'),
                          ((64, 2, 1, 0, 4, 4), b'align must be a power of two in [1, 4096]'),
                          ((64, 2, 1, 12, 4, 4), b'align must be a power of two'),
                          ((64, 2, 1, 8192, 4, 4), b'align must be a power of two'),
                          ((64, 2, 1, 1, -1, 4), b'max_segments must not be negative'),
                          ((64, 2, 1, 1, 4, -1), b'capacity must lie in [0, n]'),
                          ((64, 2, 1, 1, 4, 65), b'capacity must lie in [0, n]'),
                          ((2**31 - 1, 2**31 - 1, 1, 1, 0, 0), b'too large for one launch')):
        assert lib.wfk_segment_rows_plan_create(*args, C.byref(h)) == -1 and not h
        err = lib.wfk_last_error()
        assert err.startswith(b'segment rows plan: ') and message in err, err
    assert lib.wfk_segment_rows_plan_create(64, 2, 1, 1, 4, 4, None) == -1
    assert lib.wfk_segment_rows_apply_bit(None, None, 0, 0, None, 0, None, 0, None, None) == -1
    assert lib.wfk_segment_rows_apply_marks(None, None, 0, None, 0, None, 0, None, 0, None, None) == -1
    assert lib.wfk_segment_rows_span(None) == 0 and lib.wfk_segment_rows_kernel_name(None, 0, 0) == b''
    assert lib.wfk_segment_rows_plan_destroy(None) == 0


BUILDS = {'plain': ['-O3'],
          'sanitized': ['-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan']}


@pytest.mark.parametrize('build', list(BUILDS))
def test_the_row_rule_holds_the_stage_to_its_lines(build, tmp_path):
    exe = tmp_path / f'segment_row_rule_{build}'
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', *BUILDS[build],
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'waveforms_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'segment_row_rule_host.cpp'), '-o', str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == 'segment row rule ok' and not r.stderr, (r.stdout, r.stderr)
