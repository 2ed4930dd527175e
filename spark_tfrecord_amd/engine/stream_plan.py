"""Host-side planning for the streamed pipelined read (engine/gpu.py): which
byte range each arrived slice may frame-scan, how many records have fully
arrived, and how large the row-indexed buffers must be. Pure arithmetic, no
GPU: every capacity a kernel writes through is decided here, on the host,
before the launch."""

from __future__ import annotations

from typing import List, NamedTuple

# a frame is at least 16 bytes (length, length CRC, empty payload, data CRC)
MIN_FRAME = 16
# candidate windows read up to 32 bytes ahead of their position
SCAN_LOOKAHEAD = 32


class SlicePlan(NamedTuple):
    b0: int       # first byte of the slice
    b1: int       # one past its last byte == bytes arrived once it has landed
    scan_lo: int  # candidate positions [scan_lo, scan_hi) are scanned when
    scan_hi: int  # this slice lands (empty when scan_hi == scan_lo)


def plan_slices(n: int, span: int) -> List[SlicePlan]:
    """Cut an n-byte file into H2D slices of `span` bytes. Positions within
    SCAN_LOOKAHEAD bytes of a slice end are deferred to the next slice (their
    load window crosses the boundary); the last slice scans to the end. The
    scan ranges tile [0, n) exactly, in order."""
    if n <= 0:
        return []
    span = max(1, int(span))
    S = (n + span - 1) // span
    out = []
    scanned = 0
    for s in range(S):
        b0, b1 = s * span, min(n, (s + 1) * span)
        hi = b1 - SCAN_LOOKAHEAD if s < S - 1 else n
        hi = max(hi, scanned)
        out.append(SlicePlan(b0, b1, scanned, hi))
        scanned = hi
    return out


def arrived_records(n_cand: int, last_end: int, arrived: int) -> int:
    """Of n_cand chained candidates, how many lie entirely inside the first
    `arrived` bytes. In an unbroken chain every candidate but the last ends
    where its successor starts, i.e. below the scanned range's end, so only
    the last one (ending at last_end) can still be in flight."""
    if n_cand <= 0:
        return 0
    return n_cand if last_end <= arrived else n_cand - 1


def launchable_records(n_cand: int, last: bool) -> int:
    """Of n_cand chained candidates, how many a slice's launches may cover
    without the host reading the chain end first. Before the last slice the
    last candidate always waits for the next slice (one record of deferral
    per slice): every other one ends where its successor starts, i.e. below
    the scanned range's end. After the last slice all of them have arrived."""
    if n_cand <= 0:
        return 0
    return n_cand if last else n_cand - 1


def row_capacity(need: int, bytes_seen: int, total_bytes: int,
                 headroom: float, min_unit: int = MIN_FRAME) -> int:
    """Capacity, in rows, for a file of total_bytes of which bytes_seen held
    `need` rows: that density extrapolated to the whole file, times
    `headroom`. Never below `need`, never above what the unseen bytes can
    still hold at min_unit bytes a row (a record takes MIN_FRAME bytes; a
    decoded value, payload byte or sub-list at least one)."""
    need = max(int(need), 0)
    bytes_seen = min(max(int(bytes_seen), 1), max(int(total_bytes), 1))
    est = int(need * (total_bytes / bytes_seen) * max(headroom, 1.0)) + 1
    most = need + max(total_bytes - bytes_seen, 0) // max(min_unit, 1)
    return max(need, min(est, most), 1)


def grown_capacity(cap: int, need: int, bytes_seen: int, total_bytes: int,
                   headroom: float, min_unit: int = MIN_FRAME) -> int:
    """Capacity after a launch that needs `need` rows: unchanged while it
    fits, else re-planned from the density seen so far (the new estimate
    again covers the rest of the file, so regrows stay rare)."""
    if need <= cap:
        return cap
    return row_capacity(need, bytes_seen, total_bytes, headroom, min_unit)
