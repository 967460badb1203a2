"""`distortion.SampledIirRows` without a device: its argument errors come before any device call, and the padding of
`_engine.pack_sections_rows` shows in `own_orders` / `section_order` / `row_state`."""
import numpy as np
import pytest

import waveforms_amd as wf
from waveforms_amd import _engine, distortion, workloads as wl
from waveforms_amd.distortion import SampledIirRows, exp_decay_filter

GRID = wl.awg_grid(2000, 2e9)
FO = lambda A, tau: exp_decay_filter(A, tau, 2e9)      # one first-order section


def _chans(rows):
    return [wl.awg_channel(wf, c, 2000, 2e9) for c in range(rows)]


@pytest.fixture
def no_device(monkeypatch):
    """any call that would reach the device fails the test"""
    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_engine, 'DeviceBuffer', boom)
    monkeypatch.setattr(_engine, 'sync', boom)


def test_value_errors_before_any_device_call(no_device, monkeypatch):
    monkeypatch.setattr(_engine, 'ChainIirRowsPlan', lambda *a, **k: pytest.fail('a plan was created'))
    with pytest.raises(ValueError, match='3 cascades for 2 rows'):
        SampledIirRows(_chans(2), GRID, [[FO(0.02, 150e-9)]] * 3)
    with pytest.raises(ValueError, match='1 cascades for 4 rows'):
        SampledIirRows(_chans(2), GRID, [[FO(0.02, 150e-9)]], tile=2)
    with pytest.raises(ValueError, match='without sections'):
        SampledIirRows(_chans(2), GRID, [[FO(0.02, 150e-9)], []])
    for dtype in (np.float16, np.complex128, np.int32):
        with pytest.raises(ValueError, match='float64 or float32'):
            SampledIirRows(_chans(1), GRID, [[FO(0.02, 150e-9)]], dtype=dtype)
    with pytest.raises(NotImplementedError, match='complex'):
        SampledIirRows(_chans(1), GRID, [[([1.0, 0.5j], [1.0, -0.9])]])


@pytest.mark.parametrize('cascade,what', [
    ([(0.01, 20e-9), (0.02, 200e-9), (-0.015, 1e-6), (0.01, 5e-6), (0.02, 80e-9)], 'five first-order sections'),
    ('mixed', 'an order-1 next to an order-3 section: padded to two sections of order 3'),
    ('three_biquads', 'three biquads'),
])
def test_shapes_beyond_the_limit_name_it(no_device, cascade, what):
    """the library refuses the shape before it looks for a device (so this holds with and without one)"""
    if cascade == 'mixed':
        secs = [FO(0.02, 150e-9), ([1.0, 0.2, 0.1, 0.05], [1.0, -0.5, 0.1, -0.01])]
    elif cascade == 'three_biquads':
        secs = [([1.0, 0.2, 0.1], [1.0, -0.5, 0.1])] * 3
    else:
        secs = [FO(A, tau) for A, tau in cascade]
    with pytest.raises(NotImplementedError, match='state dimension <= 4'):
        SampledIirRows(_chans(2), GRID, [[FO(0.02, 150e-9)], secs])


class _StubPlan:
    """stands in for _engine.ChainIirRowsPlan: what the class reads of a plan, no library call"""

    def __init__(self, prog, grid, sections_per_row, dtype, packed=None):
        orders, bm, am, own = _engine.pack_sections_rows(sections_per_row) if packed is None else packed
        self.packed = (orders, bm, am, own)
        self.n, self.n_channels, self.state_dim = int(grid.n), prog.n_channels, int(orders.sum())
        self.fused, self.why_not = False, 'a stub'

    def kernel_name(self):
        return 'stub'

    def close(self):
        pass


def test_padding_shows_in_own_orders_and_section_order(monkeypatch):
    monkeypatch.setattr(_engine, 'ChainIirRowsPlan', _StubPlan)
    biquad = ([1.0, 0.2, 0.1], [1.0, -0.5, 0.1])
    rows = [[FO(0.02, 150e-9)], [biquad, FO(-0.01, 1.5e-6)], [([2.0], [1.0, -0.5])]]
    sr = SampledIirRows(_chans(3), GRID, rows, dtype=np.float32)
    assert (sr.n, sr.n_channels, sr.dtype) == (2000, 3, np.dtype(np.float32))
    # every section padded to the widest order of any row (2), every row to the largest section count (2)
    assert sr.section_order == 2 and sr.state_dim == 4
    assert sr.own_orders == [[1], [2, 1], [1]]
    orders, bm, am, _ = sr.plan.packed
    assert list(orders) == [2, 2] and bm.shape == am.shape == (3, 6)
    b0, a0 = rows[0][0]
    assert np.array_equal(bm[0], [b0[0], b0[1], 0, 1, 0, 0]) and np.array_equal(am[0], [a0[0], a0[1], 0, 1, 0, 0])
    assert np.array_equal(bm[2], [2, 0, 0, 1, 0, 0]) and np.array_equal(am[2], [1, -0.5, 0, 1, 0, 0])
    # a row's own state out of the padded (rows, state_dim) layout: section s at s * section_order, its own order long
    z = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(sr.row_state(z, 0), [0.0])
    assert np.array_equal(sr.row_state(z, 1), [4.0, 5.0, 6.0])
    assert np.array_equal(sr.row_state(z, 2), [8.0])
    assert sr.kernel_name() == 'stub' and not sr.fused and sr.why_not
    sr.close()
    # tile repeats the channel list: one cascade per RESULTING row
    sr = SampledIirRows(_chans(3), GRID, rows * 2, tile=2)
    assert sr.n_channels == 6 and sr.own_orders == [[1], [2, 1], [1]] * 2
    assert isinstance(sr, distortion.SampledIirRows)
