"""The mix stage (distortion.MixStage / mix_rows), everything up to the point a device is needed: the referee's own
properties (tests/mix_rows_ref.py), the builder of order- and contraction-sensitive rows held to exact rational
arithmetic, the argument checks that come before any device work at all three levels, the read count of the tiling,
and the declarations of the header."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import mix_rows_ref as ref
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _engine.MIX_TILE_ROWS


class Csr:
    """what `.tocsr()` of a scipy.sparse matrix gives, as far as the stage reads it: lets a test hand over index arrays
    that a dense matrix cannot produce"""

    def __init__(self, shape, indptr, indices, data):
        self.shape, self.indptr, self.indices, self.data = shape, np.array(indptr), np.array(indices), np.array(data, dtype=float)

    def tocsr(self):
        return self


# ---- the referee ---------------------------------------------------------------------------------------------------------
def test_referee_permutation_moves_rows_bit_for_bit():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 300)) * 10.0**rng.integers(-300, 300, (5, 300))
    x[x == 0.0] = 1.0
    m, perm = ref.permutation(5, 1)
    assert not np.array_equal(perm, np.arange(5))
    assert ref.mix_ref(x, m).tobytes() == x[perm].tobytes()            # 0.0 + x * 1.0 == x for every non-zero finite x
    with np.errstate(over='ignore'):
        x32 = x.astype(np.float32)
    x32[(x32 == 0.0) | ~np.isfinite(x32)] = 1.0
    assert ref.mix_ref(x32, m).tobytes() == x32[perm].tobytes()


def test_referee_identity_offset_and_rows_without_terms():
    x = ref.rows_input(4, 50, 2, specials=False)
    off = np.array([0.5, -1.25, 0.0, 3.0])
    assert np.array_equal(ref.mix_ref(x, np.eye(4), off), x + off[:, None])
    m = np.eye(4)
    m[2] = 0.0
    y = ref.mix_ref(x, m, off)
    assert np.all(y[2] == 0.0) and not np.signbit(y[2]).any() and np.array_equal(y[3], x[3] + 3.0)
    assert np.all(ref.mix_ref(x, np.zeros((2, 4)), [7.0, -0.0]) == np.array([[7.0], [0.0]]))
    assert not np.signbit(ref.mix_ref(x, np.zeros((1, 4)), [-0.0])).any()        # fl(0.0 + -0.0) is +0.0


def test_referee_keeps_nan_and_inf_out_of_rows_without_a_term_on_them():
    x = ref.rows_input(3, 64, 3, specials=False)
    x[1] = np.nan
    x[2, ::2] = np.inf
    m = np.array([[1.0, 0.0, 0.0], [1.0, 2.0, 0.0], [0.5, 0.0, 0.25], [0.0, 0.0, -1.0]])
    y = ref.mix_ref(x, m)
    assert np.all(np.isfinite(y[0])) and np.all(np.isnan(y[1]))
    assert np.all(np.isinf(y[2, ::2])) and np.all(np.isfinite(y[2, 1::2])) and np.all(y[3, ::2] == -np.inf)
    with np.errstate(all='ignore'):
        assert np.all(np.isnan(m @ x)[0])                                        # what a dense product makes of it


def test_referee_rounds_float32_once():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 4000)).astype(np.float32)
    m = np.array([[0.3, -0.7, 1.1]])
    y = ref.mix_ref(x, m, [0.1])
    assert y.dtype == np.float32
    x64 = x.astype(np.float64)
    once = (((0.0 + x64[0] * 0.3) + x64[1] * -0.7) + x64[2] * 1.1 + 0.1).astype(np.float32)
    assert y[0].tobytes() == once.tobytes()
    each = np.float32(0.0)
    for c in range(3):
        each = (each + (x[c] * np.float32(m[0, c])).astype(np.float32)).astype(np.float32)
    assert np.count_nonzero((each + np.float32(0.1)).astype(np.float32) != y[0]) > 100     # rounding every step differs


def test_sensitive_rows_change_under_another_order_or_a_fused_multiply_add():
    x, m = ref.sensitive_case(512, seed=3)
    assert x.shape == (3, 512) and m.shape == (1, 3) and np.all(m != 0)
    y = ref.mix_ref(x, m)[0]
    for i in range(512):
        xi = x[:, i]
        p = [float(Fraction(float(xi[c])) * Fraction(float(m[0, c]))) for c in range(3)]     # the rounded products
        assert p == [float(xi[c]) * float(m[0, c]) for c in range(3)]
        asc = float(Fraction(float(Fraction(p[0]) + Fraction(p[1]))) + Fraction(p[2]))       # (0.0 + p0 is p0: p0 != 0)
        desc = float(Fraction(float(Fraction(p[2]) + Fraction(p[1]))) + Fraction(p[0]))
        assert y[i] == asc and asc != desc and asc != ref.fused(xi, m[0])
    # the same through the referee: the matrix with its columns reversed sums the same products in the other order
    assert np.all(ref.mix_ref(x[::-1], m[:, ::-1])[0] != y)


# ---- refusals: MixStage, mix_rows_arguments, mix_rows --------------------------------------------------------------------
BAD = [   # (matrix, offset, n, dtype, exception, message)
    (np.zeros(4), None, 8, np.float64, ValueError, 'matrix must be 2-D'),
    (np.zeros((2, 2, 2)), None, 8, np.float64, ValueError, 'matrix must be 2-D'),
    (np.zeros((0, 3)), None, 8, np.float64, ValueError, 'rows_out < 1'),
    (np.zeros((3, 0)), None, 8, np.float64, ValueError, 'rows_in < 1'),
    (np.eye(3), None, -1, np.float64, ValueError, 'n < 0'),
    (np.eye(3), [0.0, 1.0], 8, np.float64, ValueError, 'offset: one per output row'),
    (np.eye(3), [0.0, 1.0, 2.0, 3.0], 8, np.float64, ValueError, 'offset: one per output row'),
    (np.eye(3), [0.0, np.inf, 0.0], 8, np.float64, ValueError, 'row 1: offset is not finite'),
    (np.eye(3), [0.0, 0.0, np.nan], 8, np.float64, ValueError, 'row 2: offset is not finite'),
    (np.array([[1.0, 0.0], [np.nan, 1.0]]), None, 8, np.float64, ValueError, r'row 1: coefficient \(1, 0\) is not finite'),
    (np.array([[1.0, -np.inf], [0.0, 1.0]]), None, 8, np.float64, ValueError, r'row 0: coefficient \(0, 1\) is not finite'),
    (Csr((2, 3), [0, 1, 2], [0, 3], [1.0, 1.0]), None, 8, np.float64, ValueError, 'row 1: column 3 is out of range'),
    (Csr((2, 3), [0, 1, 2], [-1, 2], [1.0, 1.0]), None, 8, np.float64, ValueError, 'row 0: column -1 is out of range'),
    (Csr((2, 3), [0, 2, 3], [2, 1, 0], [1.0, 1.0, 1.0]), None, 8, np.float64, ValueError, 'row 0: columns are not ascending'),
    (Csr((2, 3), [0, 1, 3], [0, 1, 1], [1.0, 1.0, 1.0]), None, 8, np.float64, ValueError, 'row 1: columns are not ascending'),
    (Csr((2, 3), [1, 1, 2], [0, 1], [1.0, 1.0]), None, 8, np.float64, ValueError, 'row_ptr is not non-decreasing from 0'),
    (Csr((2, 3), [0, 2, 1], [0, 1], [1.0, 1.0]), None, 8, np.float64, ValueError, 'row_ptr is not non-decreasing from 0'),
    (np.eye(3), None, 8, np.int16, ValueError, 'dtype must be float64 or float32'),
    (np.eye(3), None, 8, np.float16, ValueError, 'dtype must be float64 or float32'),
    (np.eye(3), None, 8, np.complex128, NotImplementedError, 'complex'),
    (np.eye(3), None, 8, np.complex64, NotImplementedError, 'complex'),
]


@pytest.mark.parametrize('matrix,offset,n,dtype,exc,message', BAD, ids=[f'{i}-{b[5][:24]}' for i, b in enumerate(BAD)])
def test_stage_and_arguments_refuse_before_any_device_work(matrix, offset, n, dtype, exc, message):
    with pytest.raises(exc, match=message):
        _engine.mix_rows_arguments(matrix, offset, n, dtype)
    with pytest.raises(exc, match=message):
        distortion.MixStage(matrix, n, offset=offset, dtype=dtype)
    with pytest.raises(exc, match=message):
        _engine.MixRowsPlan(matrix, offset, n, dtype)


def test_from_blocks_refuses_before_any_device_work():
    with pytest.raises(ValueError, match='blocks'):
        distortion.MixStage.from_blocks([], 8)
    with pytest.raises(ValueError, match='blocks'):
        distortion.MixStage.from_blocks([[1.0, 2.0]], 8)
    with pytest.raises(ValueError, match=r'row 2: coefficient \(2, 3\) is not finite'):
        distortion.MixStage.from_blocks([np.eye(2), [[1.0, np.nan], [0.0, 1.0]]], 8)
    with pytest.raises(ValueError, match='offset: one per output row'):
        distortion.MixStage.from_blocks([np.eye(2), np.eye(2)], 8, offset=[0.0, 0.0])
    blocks, off = ref.iq_blocks(3, 5)
    assert np.array_equal(distortion.MixStage.block_diagonal(blocks), ref.block_diagonal(blocks))
    assert distortion.MixStage.block_diagonal([np.ones((1, 2)), np.ones((2, 1))]).tolist() == [[1, 1, 0], [0, 0, 1], [0, 0, 1]]


def test_arguments_are_the_terms_in_csr_form():
    m = np.array([[0.0, 2.0, 0.0, -0.0], [0.0, 0.0, 0.0, 0.0], [1.5, 0.0, 0.0, -3.0]])
    row_ptr, col, val, off, n, dtype = _engine.mix_rows_arguments(m, None, 16, np.float32)
    assert (row_ptr.dtype, col.dtype, val.dtype, off.dtype) == (np.int64, np.int32, np.float64, np.float64)
    assert row_ptr.tolist() == [0, 1, 1, 3] and col.tolist() == [1, 0, 3] and val.tolist() == [2.0, 1.5, -3.0]
    assert off.tolist() == [0.0, 0.0, 0.0] and n == 16 and dtype == np.dtype(np.float32)
    # stored zeros are accepted and dropped: they are not terms
    stored = Csr((3, 4), [0, 2, 3, 5], [1, 3, 2, 0, 3], [2.0, 0.0, -0.0, 1.5, -3.0])
    got = _engine.mix_rows_arguments(stored, [1.0, 2.0, 3.0], 16, np.float64)
    assert got[0].tolist() == [0, 1, 1, 3] and got[1].tolist() == [1, 0, 3] and got[2].tolist() == [2.0, 1.5, -3.0]
    assert got[3].tolist() == [1.0, 2.0, 3.0]
    if _engine.importlib.util.find_spec('scipy') is not None:
        import scipy.sparse as sp
        for form in (sp.csr_matrix(m), sp.coo_matrix(m), sp.csc_matrix(m)):
            got = _engine.mix_rows_arguments(form, None, 16, np.float64)
            assert got[0].tolist() == [0, 1, 1, 3] and got[1].tolist() == [1, 0, 3] and got[2].tolist() == [2.0, 1.5, -3.0]


def test_wrapper_refuses_and_handles_empty_rows_without_a_device():
    with pytest.raises(ValueError, match='2-D'):
        distortion.mix_rows(np.zeros(16), np.eye(1))
    with pytest.raises(ValueError, match='2-D'):
        distortion.mix_rows(np.zeros((2, 2, 4)), np.eye(2))
    with pytest.raises(NotImplementedError):
        distortion.mix_rows(np.zeros((2, 4)) + 0j, np.eye(2))
    with pytest.raises(ValueError, match='3 columns for 2 rows'):
        distortion.mix_rows(np.zeros((2, 4)), np.eye(3))
    with pytest.raises(ValueError, match='matrix must be 2-D'):
        distortion.mix_rows(np.zeros((2, 4)), np.zeros(2))
    with pytest.raises(ValueError, match='row 0: offset is not finite'):
        distortion.mix_rows(np.zeros((2, 4)), np.eye(2), [np.nan, 0.0])
    with pytest.raises(ValueError, match='offset: one per output row'):
        distortion.mix_rows(np.zeros((2, 0)), np.eye(2), [0.0])
    y = distortion.mix_rows(np.zeros((3, 0)), np.ones((5, 3)), np.arange(5.0))        # nothing to mix: no device needed
    assert y.shape == (5, 0) and y.dtype == np.float64
    y = distortion.mix_rows(np.zeros((3, 0), dtype=np.float32), np.ones((2, 3)))
    assert y.shape == (2, 0) and y.dtype == np.float32
    assert distortion.mix_rows(np.zeros((3, 0), dtype=np.int32), np.ones((2, 3))).dtype == np.float64


# ---- the library itself -------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_mix_rows_plan_create', 'wfk_mix_rows_apply', 'wfk_mix_rows_reads', 'wfk_mix_rows_kernel_name',
                 'wfk_mix_rows_plan_destroy'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_mix_rows_plan wfk_mix_rows_plan;' in src
    assert int(re.search(r'#define WFK_MIX_TILE_ROWS (\d+)', src).group(1)) == _engine.MIX_TILE_ROWS
    assert lib.wfk_abi_version() == 2
    for name in ('MixStage', 'mix_rows'):
        assert hasattr(distortion, name)
    for name in ('MixRowsPlan', 'mix_rows_arguments', 'mix_rows_reads', 'MIX_TILE_ROWS'):
        assert hasattr(_engine, name)
    assert issubclass(_engine.MixRowsPlan, _engine._Handle)


def test_library_refuses_before_any_device_work():
    """the C side's own refusals come before it looks for a device: WFK_EINVAL (-1) here, with the row named"""
    lib = _engine.lib()
    create = lib.wfk_mix_rows_plan_create
    I64, I32, D = C.c_int64, C.c_int32, C.c_double
    h = C.c_void_p()

    def refused(message, n=64, rows_out=2, rows_in=3, kind=0, row_ptr=(0, 1, 3), col=(0, 1, 2), val=(1.0, 2.0, 3.0),
                offset=(0.0, 0.0), out=True):
        rp = (I64 * len(row_ptr))(*row_ptr) if row_ptr is not None else None
        cc = (I32 * max(len(col), 1))(*col) if col is not None else None
        vv = (D * max(len(val), 1))(*val) if val is not None else None
        oo = (D * len(offset))(*offset) if offset is not None else None
        rc = create(n, rows_out, rows_in, kind, rp, cc, vv, oo, C.byref(h) if out else None)
        assert rc == -1 and not h, (message, rc)
        assert message.encode() in lib.wfk_last_error(), (message, lib.wfk_last_error())

    refused('row 1: column 3 is out of range', col=(0, 1, 3))
    refused('row 0: column -1 is out of range', col=(-1, 1, 2))
    refused('row 1: columns are not ascending', col=(0, 2, 1))
    refused('row 1: columns are not ascending', col=(0, 1, 1))
    refused('row 1: coefficient (1, 2) is not finite', val=(1.0, 2.0, float('nan')))
    refused('row 0: coefficient (0, 0) is not finite', val=(float('inf'), 2.0, 3.0))
    refused('row 1: offset is not finite', offset=(0.0, float('-inf')))
    refused('row 0: offset is not finite', offset=(float('nan'), 0.0))
    refused('row_ptr is not non-decreasing from 0', row_ptr=(1, 1, 3))
    refused('row_ptr is not non-decreasing from 0', row_ptr=(0, 3, 2))
    refused('rows_out < 1', rows_out=0)
    refused('rows_in < 1', rows_in=0)
    refused('n < 0', n=-1)
    for kind in (2, 3, -1, 7):
        refused('kind must be F64 or F32', kind=kind)
    refused('too large for one launch', n=2**62)
    refused('too large for one launch', n=2**62, kind=1)
    refused('null', row_ptr=None)
    refused('null', col=None)
    refused('null', val=None)
    refused('null', out=False)
    # refused for its arguments, not for the device: zeros in val and a null offset pass every check above
    assert lib.wfk_mix_rows_apply(None, None, 64, None, 64, None) == -1
    assert b'null plan' in lib.wfk_last_error()
    assert lib.wfk_mix_rows_plan_destroy(None) == 0
    assert lib.wfk_mix_rows_kernel_name(None) == b''
    assert lib.wfk_mix_rows_reads(None) == 0


# ---- .reads: what the tiling reads ------------------------------------------------------------------------------------------
def reads(matrix):
    row_ptr, col = _engine.mix_rows_arguments(matrix, None, 64, np.float64)[:2]
    got = _engine.mix_rows_reads(row_ptr, col)
    assert got == ref.reads_of(matrix, T)
    return got


def test_reads_of_blocks_bands_and_dense_matrices():
    assert T == 8
    assert reads(ref.block_diagonal(ref.iq_blocks(T, 1)[0])) == 2 * T               # 2 x 2 blocks on 2 T rows: rows_in
    tri = ref.band(3 * T, 1, 2)
    assert np.count_nonzero(tri) == 3 * 3 * T - 2
    assert reads(tri) == 3 * T + 4                                                  # two tile edges, a row across each way
    assert reads(ref.band(4 * T, 4, 3)) == 4 * T + 3 * 2 * 4
    assert reads(ref.dense(2 * T, 5, 4)) == 10
    assert reads(ref.dense(2 * T + 1, 5, 4)) == 15                                  # a partial tile reads them again
    hole = ref.band(3 * T, 1, 5)
    hole[T:2 * T] = 0.0                                                             # a tile without terms reads nothing
    assert reads(hole) == (T + 1) + 0 + (T + 1)
    assert reads(np.zeros((3, 4))) == 0
    assert reads(ref.one_long_row(T + 2, 40, 3, 6)) == 40 + 2
    assert reads(np.eye(1)) == 1
