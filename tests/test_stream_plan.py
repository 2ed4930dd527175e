"""Host-side planner of the streamed pipelined read (no GPU needed)."""

import pytest

from spark_tfrecord_amd.engine import stream_plan as sp


@pytest.mark.parametrize("n,span", [
    (1, 4096), (31, 4096), (4096, 4096), (4097, 4096), (100_000, 4096),
    (215_000_000, 48 << 20), (1000, 16), (1000, 1), (65, 32), (64, 33),
])
def test_scan_ranges_tile_the_file(n, span):
    plan = sp.plan_slices(n, span)
    assert len(plan) == (n + span - 1) // span
    pos = 0
    for s, p in enumerate(plan):
        assert p.b0 == s * span and p.b1 == min(n, (s + 1) * span)
        assert p.scan_lo == pos and p.scan_hi >= p.scan_lo
        last = s == len(plan) - 1
        # a candidate window reads SCAN_LOOKAHEAD bytes past its position:
        # nothing beyond the arrived bytes unless this is the last slice
        assert last or p.scan_hi + sp.SCAN_LOOKAHEAD <= p.b1 or \
            p.scan_hi == p.scan_lo
        pos = p.scan_hi
    assert pos == n


def test_empty_file_has_no_slices():
    assert sp.plan_slices(0, 4096) == []


def test_deferral_at_slice_boundary():
    plan = sp.plan_slices(10_000, 4096)
    assert [(p.scan_lo, p.scan_hi) for p in plan] == \
        [(0, 4064), (4064, 8160), (8160, 10_000)]


def test_arrived_records():
    assert sp.arrived_records(0, 0, 100) == 0
    assert sp.arrived_records(5, 100, 100) == 5   # ends exactly on the boundary
    assert sp.arrived_records(5, 101, 100) == 4   # last one straddles
    assert sp.arrived_records(1, 6000, 4096) == 0  # slice smaller than a record


def test_row_capacity_extrapolates_density():
    # 1000 rows in the first quarter -> ~4000 rows, plus headroom
    cap = sp.row_capacity(1000, 250_000, 1_000_000, 1.125)
    assert 4500 <= cap <= 4501
    # never below what is needed now
    assert sp.row_capacity(1000, 1_000_000, 1_000_000, 1.0) >= 1000
    assert sp.row_capacity(0, 10, 1000, 1.125) >= 1
    # never above what the unseen bytes can hold
    assert sp.row_capacity(10, 100, 260, 100.0) == 10 + 160 // sp.MIN_FRAME
    assert sp.row_capacity(10, 100, 260, 100.0, min_unit=1) == 10 + 160
    # headroom below 1 is not a shrink factor
    assert sp.row_capacity(100, 500, 1000, 0.1, min_unit=1) >= 200


def test_grown_capacity():
    assert sp.grown_capacity(100, 100, 10, 1000, 1.125) == 100  # fits
    grown = sp.grown_capacity(100, 101, 500, 1000, 1.125)
    assert grown >= 101 and grown == sp.row_capacity(101, 500, 1000, 1.125)
    # density jump: tiny records after a sparse start still fit after regrow
    assert sp.grown_capacity(3, 400, 8192, 16384, 1.0) >= 400
