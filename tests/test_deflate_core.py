"""CPU tests of the device DEFLATE compressor core (csrc/deflate_core.h).

The code that runs one-segment-per-wave on the GPU also compiles for the
host (`_native.host_deflate_segment` emulates the lanes with a loop and is
byte-identical to the device), so the algorithm is tested here: every
produced segment must inflate back to its input under zlib AND under the
project's own inflater core, stay within its output bound, and a whole
image assembled from host-core segments must be a valid gzip file that
carries the right segment table."""

import gzip
import zlib

import pytest

import deflate_cases as C
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P

CASES = C.cases()


def check_segments(data: bytes, seg: int, threshold=None):
    """The four per-segment checks; returns the segment bodies."""
    parts = C.split(data, seg)
    bodies = C.host_segments(data, seg, threshold)
    for i, (part, body) in enumerate(zip(parts, bodies)):
        d = zlib.decompressobj(-15)
        got = d.decompress(body) + d.flush()
        assert got == part, f"zlib, segment {i}"
        assert d.unused_data == b""
        assert d.eof == (i == len(parts) - 1), f"BFINAL, segment {i}"
        assert _native.host_inflate_segment(body, len(part)) == part, \
            f"inflate core, segment {i}"
        assert len(body) <= C.seg_out_bound(len(part)), f"bound, segment {i}"
        if i < len(parts) - 1:
            assert body.endswith(b"\x00\x00\xff\xff"), f"marker, segment {i}"
    return bodies


@pytest.mark.parametrize("name,data,seg", CASES, ids=[c[0] for c in CASES])
def test_roundtrip_and_image(name, data, seg):
    bodies = check_segments(data, seg)
    img = C.host_gzip_image(data, seg)
    assert gzip.decompress(img) == data  # verifies CRC-32 and ISIZE
    meta = P.parse_gz_segments(img)
    assert meta is not None
    body_off, segs, crc, isize = meta
    parts = C.split(data, seg)
    assert body_off == 20 + 8 * len(parts)
    assert segs == [(len(b), len(p)) for b, p in zip(bodies, parts)]
    assert crc == zlib.crc32(data) & 0xFFFFFFFF
    assert isize == len(data)
    assert P._gunzip_parallel(img) == data
    # determinism: a second host run is byte-identical
    assert C.host_segments(data, seg) == bodies


@pytest.mark.parametrize("name,data,seg", CASES, ids=[c[0] for c in CASES])
def test_never_above_stored(name, data, seg):
    # the encoding is chosen by minimum cost, threshold or not
    for thr in (P._GZ_STORED_THRESHOLD, 0.0):
        parts = C.split(data, seg)
        for i, (part, body) in enumerate(
                zip(parts, check_segments(data, seg, thr))):
            u = len(part)
            stored = (5 if u == 0 else
                      u + 5 * (-(-u // 65535)) + (0 if i == len(parts) - 1 else 5))
            assert len(body) <= stored


def _block_types(body: bytes):
    """BTYPE of the first block (the core emits one Huffman block, or
    stored blocks only)."""
    return (body[0] >> 1) & 3


def test_paths_taken():
    by = {c[0]: c for c in CASES}
    seg0 = lambda n: C.host_segments(by[n][1], by[n][2])[0]
    assert _block_types(seg0("random128k")) == 0       # stored
    assert len(seg0("random128k")) == (128 << 10) + 5 * 3  # three blocks
    assert _block_types(seg0("alpha25")) == 2          # dynamic
    assert _block_types(seg0("no_trigram_repeat")) == 2
    assert _block_types(seg0("one_literal")) == 2
    assert _block_types(seg0("len0")) == 1             # fixed: just EOB
    assert seg0("len0") == b"\x03\x00"
    assert _block_types(seg0("distinct256")) == 0


def test_stored_threshold_semantics():
    data = [c for c in CASES if c[0] == "alpha25"][0][1]
    huff = _native.host_deflate_segment(data, True, 0.98)
    assert len(huff) < 0.98 * len(data)
    # the same segment under a threshold its best encoding misses
    below = (len(huff) - 0.5) / len(data)
    stored = _native.host_deflate_segment(data, True, below)
    assert len(stored) == len(data) + 5 and stored[0] == 1
    assert _native.host_deflate_segment(data, True, 0.0) == huff
    above = (len(huff) + 0.5) / len(data)
    assert _native.host_deflate_segment(data, True, above) == huff


def test_size_of_a_long_run():
    # fixed codes: a 258-match at distance 1 is 13 bits, so max-length
    # matches give ~215 bytes and a parse cut every 64 positions ~832;
    # above 1024 the matcher or the cost choice is broken
    body = _native.host_deflate_segment(b"\x00" * 32768, True, 0.98)
    assert len(body) <= 1024


def _kraft(lens):
    return sum(2.0 ** -l for l in lens if l)


@pytest.mark.parametrize("max_len", [15, 7])
def test_huffman_lengths(max_len):
    fib = [1, 1]
    while fib[-1] < 10946:
        fib.append(fib[-1] + fib[-2])
    assert len(fib) == 21 and fib[-1] == 10946  # unlimited depth: 20
    single = [0] * 30
    single[17] = 5
    equal = [3] * 286
    sparse = [0, 7, 0, 0, 1, 0, 2]
    for freqs in (fib, single, equal, sparse):
        if max_len == 7 and len(freqs) > 128:
            continue  # 286 codes cannot fit 7 bits
        lens = _native.host_huffman_lengths(freqs, max_len)
        assert len(lens) == len(freqs)
        used = [l for f, l in zip(freqs, lens) if f]
        assert all(l == 0 for f, l in zip(freqs, lens) if not f)
        assert all(1 <= l <= max_len for l in used)
        if len(used) >= 2:
            assert _kraft(lens) == 1.0
        else:
            assert _kraft(lens) <= 1.0
    # frequent symbols never get longer codes than rare ones
    lens = _native.host_huffman_lengths(fib, 15)
    assert lens == sorted(lens, reverse=True)
    assert max(lens) == 15
    # without a limit in reach the result is the optimal Huffman code
    lens = _native.host_huffman_lengths([5, 9, 12, 13, 16, 45], 15)
    assert sum(f * l for f, l in zip([5, 9, 12, 13, 16, 45], lens)) == 224


def test_crc32_ieee():
    for _, data, _ in CASES:
        assert _native.crc32_ieee(data) == zlib.crc32(data) & 0xFFFFFFFF
    assert _native.crc32_ieee(b"123456789") == 0xCBF43926
