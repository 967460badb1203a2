"""The fused mix-to-codes stage (distortion.MixDacStage / mix_dac_rows, csrc/wfk_mix_dac.hip) without a device: every
refusal of the two stages it is made of, with its text, at three levels (the stage, _engine.mix_dac_arguments, the C
entry through ctypes); the symbols and what they return for a NULL plan; `.reads` at the fused kernel's tile height;
and the properties of the rows the GPU test's order / contraction case rests on (tests/mix_dac_ref.py: tie_case), held
again in exact rational arithmetic."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import mix_dac_ref as ref
import mix_rows_ref
from waveforms_amd import _engine, distortion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _engine.MIX_DAC_TILE_ROWS


class Csr:
    """what `.tocsr()` of a scipy.sparse matrix gives, as far as the stage reads it"""

    def __init__(self, shape, indptr, indices, data):
        self.shape, self.indptr, self.indices, self.data = shape, np.array(indptr), np.array(indices), np.array(data, dtype=float)

    def tocsr(self):
        return self


# ---- refusals: MixDacStage, mix_dac_arguments, MixDacPlan, mix_dac_rows ------------------------------------------------
E3 = np.eye(3)
OK = dict(mix_offset=None, gain=1000.0, dac_offset=0.0, n=8, bits=16, shift=0, interleave=1, dtype=np.float64)
BAD = [   # (matrix, what differs from OK, exception, message): the mix's refusals, then the DAC's
    (np.zeros(4), {}, ValueError, 'matrix must be 2-D'),
    (np.zeros((2, 2, 2)), {}, ValueError, 'matrix must be 2-D'),
    (np.zeros((0, 3)), {}, ValueError, 'rows_out < 1'),
    (np.zeros((3, 0)), {}, ValueError, 'rows_in < 1'),
    (E3, dict(n=-1), ValueError, 'n < 0'),
    (E3, dict(mix_offset=[0.0, 1.0]), ValueError, 'offset: one per output row'),
    (E3, dict(mix_offset=[0.0, np.inf, 0.0]), ValueError, 'row 1: offset is not finite'),
    (np.array([[1.0, 0.0], [np.nan, 1.0]]), {}, ValueError, r'row 1: coefficient \(1, 0\) is not finite'),
    (Csr((2, 3), [0, 1, 2], [0, 3], [1.0, 1.0]), {}, ValueError, 'row 1: column 3 is out of range'),
    (Csr((2, 3), [0, 1, 2], [-1, 2], [1.0, 1.0]), {}, ValueError, 'row 0: column -1 is out of range'),
    (Csr((2, 3), [0, 2, 3], [2, 1, 0], [1.0, 1.0, 1.0]), {}, ValueError, 'row 0: columns are not ascending'),
    (Csr((2, 3), [1, 1, 2], [0, 1], [1.0, 1.0]), {}, ValueError, 'row_ptr is not non-decreasing from 0'),
    (E3, dict(dtype=np.int16), ValueError, 'dtype must be float64 or float32'),
    (E3, dict(dtype=np.complex128), NotImplementedError, 'complex'),
    (E3, dict(bits=1), ValueError, r'bits must lie in \[2, 16\]'),
    (E3, dict(bits=17), ValueError, r'bits must lie in \[2, 16\]'),
    (E3, dict(bits=16, shift=1), ValueError, r'shift must lie in \[0, 16 - bits\]'),
    (E3, dict(bits=12, shift=-1), ValueError, r'shift must lie in \[0, 16 - bits\]'),
    (E3, dict(interleave=0), ValueError, 'interleave must be 1 or 2'),
    (E3, dict(interleave=3), ValueError, 'interleave must be 1 or 2'),
    (E3, dict(interleave=2), ValueError, '3 rows are no multiple of the interleave 2'),
    (E3, dict(gain=[1.0, np.inf, 1.0]), ValueError, 'row 1: gain is not finite'),
    (E3, dict(gain=[np.nan, 1.0, 1.0]), ValueError, 'row 0: gain is not finite'),
    (E3, dict(dac_offset=[0.0, 0.0, -np.inf]), ValueError, 'row 2: offset is not finite'),
    # the mix's refusal comes first
    (E3, dict(n=-1, bits=1), ValueError, 'n < 0'),
    (np.zeros(4), dict(gain=[np.nan]), ValueError, 'matrix must be 2-D'),
]


@pytest.mark.parametrize('matrix,change,exc,message', BAD, ids=[f'{i}-{b[3][:24]}' for i, b in enumerate(BAD)])
def test_stage_arguments_and_plan_refuse_before_any_device_work(matrix, change, exc, message):
    a = dict(OK, **change)
    rows = np.shape(matrix)[0] if not isinstance(matrix, Csr) else matrix.shape[0]
    per_row = {k: (np.full(max(rows, 1), a[k]) if np.ndim(a[k]) == 0 else a[k]) for k in ('gain', 'dac_offset')}
    with pytest.raises(exc, match=message):
        distortion.MixDacStage(matrix, a['n'], a['gain'], mix_offset=a['mix_offset'], dac_offset=a['dac_offset'],
                               bits=a['bits'], shift=a['shift'], interleave=a['interleave'], dtype=a['dtype'])
    with pytest.raises(exc, match=message):
        _engine.mix_dac_arguments(matrix, a['mix_offset'], per_row['gain'], per_row['dac_offset'], a['n'], a['bits'],
                                  a['shift'], a['interleave'], a['dtype'])
    with pytest.raises(exc, match=message):
        _engine.MixDacPlan(matrix, a['mix_offset'], per_row['gain'], per_row['dac_offset'], a['n'], a['bits'],
                           a['shift'], a['interleave'], a['dtype'])


def test_stage_constructors_and_wrapper_refuse_before_any_device_work():
    with pytest.raises(ValueError, match='2 gain entries for 3 rows'):
        distortion.MixDacStage(E3, 8, [1.0, 2.0])
    with pytest.raises(ValueError, match='4 offset entries for 3 rows'):
        distortion.MixDacStage(E3, 8, 1.0, dac_offset=[0.0] * 4)
    with pytest.raises(ValueError, match='2 gains for 3 output rows'):
        _engine.mix_dac_arguments(E3, None, [1.0, 2.0], [0.0, 0.0], 8)
    with pytest.raises(ValueError, match='blocks'):
        distortion.MixDacStage.from_blocks([], 8, 1.0)
    with pytest.raises(ValueError, match=r'row 2: coefficient \(2, 3\) is not finite'):
        distortion.MixDacStage.from_blocks([np.eye(2), [[1.0, np.nan], [0.0, 1.0]]], 8, 1.0, interleave=2)
    with pytest.raises(ValueError, match='offset: one per output row'):
        distortion.MixDacStage.from_blocks([np.eye(2), np.eye(2)], 8, 1.0, mix_offset=[0.0, 0.0])
    for fs in (0.0, -1.0, np.inf, np.nan, [1.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match='full scale'):
            distortion.MixDacStage.from_full_scale(E3, 8, fs)
    with pytest.raises(ValueError, match='bits'):
        distortion.MixDacStage.from_full_scale(E3, 8, 1.0, bits=17)
    with pytest.raises(ValueError, match='2-D'):
        distortion.mix_dac_rows(np.zeros(16), np.eye(1), 1.0)
    with pytest.raises(NotImplementedError):
        distortion.mix_dac_rows(np.zeros((2, 4)) + 0j, np.eye(2), 1.0)
    with pytest.raises(ValueError, match='3 columns for 2 rows'):
        distortion.mix_dac_rows(np.zeros((2, 4)), np.eye(3), 1.0)
    with pytest.raises(ValueError, match='row 0: gain is not finite'):
        distortion.mix_dac_rows(np.zeros((2, 4)), np.eye(2), [np.nan, 1.0])
    with pytest.raises(ValueError, match='interleave must be 1 or 2'):
        distortion.mix_dac_rows(np.zeros((2, 4)), np.eye(2), 1.0, interleave=4)
    # nothing to mix: no device needed
    codes, counts = distortion.mix_dac_rows(np.zeros((3, 0)), np.ones((4, 3)), 1.0, interleave=2, return_counts=True)
    assert codes.shape == (2, 0) and codes.dtype == np.int16 and counts.shape == (4, 3) and not counts.any()
    assert distortion.mix_dac_rows(np.zeros((3, 0), dtype=np.float32), np.ones((4, 3)), 1.0).shape == (4, 0)


def test_arguments_are_those_of_the_two_stages():
    m = np.array([[0.0, 2.0, 0.0, -0.0], [1.5, 0.0, 0.0, -3.0]])
    got = _engine.mix_dac_arguments(m, [0.5, -0.5], [10.0, 20.0], [1.0, 2.0], 16, 14, 2, 2, np.float32)
    mix = _engine.mix_rows_arguments(m, [0.5, -0.5], 16, np.float32)
    dac = _engine.dac_rows_arguments([10.0, 20.0], [1.0, 2.0], 16, 14, 2, 2, np.float32)
    assert got[0] == 4
    for a, b in zip(got[1:5], mix[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for a, b in zip(got[5:7], dac[:2]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[7:] == (16, 14, 2, 2, np.dtype(np.float32))


# ---- the library itself -------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'wfk.h')).read()
    lib = _engine.lib()
    for name in ('wfk_mix_dac_plan_create', 'wfk_mix_dac_apply', 'wfk_mix_dac_reads', 'wfk_mix_dac_span',
                 'wfk_mix_dac_kernel_name', 'wfk_mix_dac_plan_destroy'):
        assert re.search(r'\b%s\(' % name, src), name
        assert hasattr(lib, name), name
    assert 'typedef struct wfk_mix_dac_plan wfk_mix_dac_plan;' in src
    assert int(re.search(r'#define WFK_MIX_DAC_TILE_ROWS (\d+)', src).group(1)) == T
    assert T % 2 == 0 and T <= 32                        # a pair never straddles two tiles; one mask word
    for name in ('MixDacStage', 'mix_dac_rows'):
        assert hasattr(distortion, name)
    for name in ('MixDacPlan', 'mix_dac_arguments', 'mix_dac_reads', 'MIX_DAC_TILE_ROWS'):
        assert hasattr(_engine, name)
    assert issubclass(_engine.MixDacPlan, _engine._Handle)
    # a NULL plan
    assert lib.wfk_mix_dac_apply(None, None, 64, None, 64, None, None) == -1
    assert b'null plan' in lib.wfk_last_error()
    assert lib.wfk_mix_dac_plan_destroy(None) == 0
    assert lib.wfk_mix_dac_kernel_name(None, 0) == b'' and lib.wfk_mix_dac_kernel_name(None, 1) == b''
    assert lib.wfk_mix_dac_reads(None) == 0 and lib.wfk_mix_dac_span(None) == 0


def test_library_refuses_before_any_device_work():
    """the C side's own refusals, those of wfk_mix_rows_plan_create and of wfk_dac_rows_plan_create word for word,
    come before it looks for a device: WFK_EINVAL (-1) here"""
    lib = _engine.lib()
    create = lib.wfk_mix_dac_plan_create
    I64, I32, D = C.c_int64, C.c_int32, C.c_double
    h = C.c_void_p()

    def refused(message, n=64, rows_out=2, rows_in=3, kind=0, row_ptr=(0, 1, 3), col=(0, 1, 2), val=(1.0, 2.0, 3.0),
                mix_offset=(0.0, 0.0), gain=(1.0, 1.0), dac_offset=(0.0, 0.0), bits=16, shift=0, k=1, out=True):
        rp = (I64 * len(row_ptr))(*row_ptr) if row_ptr is not None else None
        cc = (I32 * max(len(col), 1))(*col) if col is not None else None
        vv = (D * max(len(val), 1))(*val) if val is not None else None
        mo = (D * len(mix_offset))(*mix_offset) if mix_offset is not None else None
        gg = (D * len(gain))(*gain) if gain is not None else None
        do = (D * len(dac_offset))(*dac_offset) if dac_offset is not None else None
        rc = create(n, rows_out, rows_in, kind, rp, cc, vv, mo, gg, do, bits, shift, k, C.byref(h) if out else None)
        assert rc == -1 and not h, (message, rc)
        assert message.encode() in lib.wfk_last_error(), (message, lib.wfk_last_error())

    refused('row 1: column 3 is out of range', col=(0, 1, 3))
    refused('row 0: column -1 is out of range', col=(-1, 1, 2))
    refused('row 1: columns are not ascending', col=(0, 2, 1))
    refused('row 1: coefficient (1, 2) is not finite', val=(1.0, 2.0, float('nan')))
    refused('row 1: offset is not finite', mix_offset=(0.0, float('-inf')))
    refused('mix rows plan: row_ptr is not non-decreasing from 0', row_ptr=(1, 1, 3))
    refused('mix rows plan: rows_out < 1', rows_out=0)
    refused('mix rows plan: rows_in < 1', rows_in=0)
    refused('mix rows plan: n < 0', n=-1)
    for kind in (2, 3, -1, 7):
        refused('kind must be F64 or F32', kind=kind)
    refused('mix rows plan: null row_ptr', row_ptr=None)
    refused('mix rows plan: null col / val', col=None)
    refused('mix rows plan: null col / val', val=None)
    refused('null out', out=False)
    refused('bad dac rows plan arguments', gain=None)
    refused('bad dac rows plan arguments', dac_offset=None)
    refused('dac rows plan: bits must lie in [2, 16]', bits=1)
    refused('dac rows plan: bits must lie in [2, 16]', bits=17)
    refused('dac rows plan: shift must lie in [0, 16 - bits]', bits=14, shift=3)
    refused('dac rows plan: shift must lie in [0, 16 - bits]', shift=-1)
    refused('dac rows plan: interleave must be 1 or 2', k=0)
    refused('dac rows plan: interleave must be 1 or 2', k=3)
    refused('dac rows plan: 3 rows are no multiple of the interleave', rows_out=3, row_ptr=(0, 1, 3, 3),
            mix_offset=(0.0,) * 3, gain=(1.0,) * 3, dac_offset=(0.0,) * 3, k=2)
    refused('row 1: gain is not finite', gain=(1.0, float('inf')))
    refused('row 0: offset is not finite', dac_offset=(float('nan'), 0.0))
    refused('too large for one launch', n=2**62)
    refused('too large for one launch', n=2**62, kind=1, k=2)
    refused('mix rows plan: n < 0', n=-1, bits=1)                    # the mix's refusal first


# ---- .reads: what the tiling reads at the fused kernel's tile height --------------------------------------------------
def reads(matrix):
    row_ptr, col = _engine.mix_rows_arguments(matrix, None, 64, np.float64)[:2]
    got = _engine.mix_dac_reads(row_ptr, col)
    assert got == mix_rows_ref.reads_of(matrix, T)
    return got


def test_reads_of_blocks_bands_and_dense_matrices():
    assert reads(mix_rows_ref.block_diagonal(mix_rows_ref.iq_blocks(T, 1)[0])) == 2 * T       # 2 x 2 blocks: rows_in
    assert reads(mix_rows_ref.band(3 * T, 1, 2)) == 3 * T + 4                 # two tile edges, a row across each way
    assert reads(mix_rows_ref.band(4 * T, 4, 3)) == 4 * T + 3 * 2 * 4
    assert reads(mix_rows_ref.dense(2 * T, 5, 4)) == 10
    assert reads(mix_rows_ref.dense(2 * T + 1, 5, 4)) == 15                   # a partial tile reads them again
    assert reads(np.zeros((3, 4))) == 0 and reads(np.eye(1)) == 1


# ---- the rows the order / contraction case of the GPU test rests on ----------------------------------------------------
def test_tie_case_shows_the_mix_halfs_order_and_contraction_in_the_codes():
    x, m = ref.tie_case(256)
    assert x.shape == (3, 256) and m.shape == (1, 3)
    assert m[0].tolist() == mix_rows_ref.sensitive_case(1)[1][0].tolist()
    codes = []
    for i in range(x.shape[1]):
        xi = x[:, i]
        y = mix_rows_ref.ascending(xi, m[0])
        # the ascending sum, step by step in exact arithmetic rounded to double, is what the float loop gives
        acc = 0.0
        for xc, mc in zip(xi, m[0]):
            p = float(Fraction(float(xc)) * Fraction(float(mc)))
            acc = float(Fraction(acc) + Fraction(p))
        assert acc == y and abs(y - ref.TIE_CENTRE) <= 2.0**-28
        # the converter's value is exact and a multiple of half an LSB
        v = ref.exact_v(y)
        assert (2 * v).denominator == 1 and float(y) * ref.TIE_GAIN + ref.TIE_OFFSET == float(v)
        code = ref.tie_code(y)
        want = v.numerator // v.denominator if v.denominator == 1 else None
        if want is None:                                 # a tie: half to even
            below = (2 * v - 1) // 2
            want = int(below if below % 2 == 0 else below + 1)
        assert code == want and abs(code) <= 32000
        assert ref.tie_code(ref.descending(xi, m[0])) != code
        assert ref.tie_code(mix_rows_ref.fused(xi, m[0])) != code
        codes.append(code)
    got, counts = ref.mix_dac_ref(x, m, None, ref.TIE_GAIN, ref.TIE_OFFSET)
    assert got[0].tolist() == codes and not counts.any()
    assert len(set(codes)) >= 200
