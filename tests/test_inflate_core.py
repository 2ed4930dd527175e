"""CPU tests of the device DEFLATE inflater core (csrc/inflate_core.h).

The exact code that runs one-segment-per-wave on the GPU also compiles for
the host (`_native.host_inflate_segment`), so the algorithm is fully
testable here: numerics vs zlib across entropy profiles, block-type
coverage (stored / fixed / dynamic), malformed-stream rejection, and the
regression for the prefetch-refill underflow (a nearly-empty prefetch
register delivered <16 bits to a 16-bit read at segment tails). The host
build takes the serial copy and table-fill paths; the lane-split ones are
covered by csrc/tests/inflate_selftest.cpp and tests/test_gpu_inflate.py."""

import gzip
import zlib

import numpy as np
import pytest

import inflate_cases as C
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P


def roundtrip(data: bytes):
    gz = P.compress_bytes(data, "gzip")
    meta = P.parse_gz_segments(gz)
    assert meta is not None
    body_off, segs, crc, isize = meta
    pos, upos = body_off, 0
    for i, (c, u) in enumerate(segs):
        out = _native.host_inflate_segment(gz[pos:pos + c], u)
        assert out == data[upos:upos + u], f"segment {i}"
        pos += c
        upos += u
    assert upos == len(data)


class TestInflateCore:
    def test_text_dynamic_huffman(self):
        rng = np.random.default_rng(0)
        roundtrip(bytes(rng.integers(65, 90, 1_500_000).astype(np.uint8)))

    def test_random_stored_blocks(self):
        roundtrip(np.random.default_rng(1).bytes(700_000))

    def test_highly_compressible(self):
        roundtrip((b"log line %08d with repeated content\n" * 20000)
                  % tuple(range(20000)))

    def test_tiny_and_empty(self):
        for d in (b"", b"a", b"ab" * 5, b"\x00" * 100):
            roundtrip(d)

    def test_exact_segment_boundaries(self):
        seg = P._GZ_SEGMENT
        rng = np.random.default_rng(2)
        for n in (seg - 1, seg, seg + 1, 2 * seg):
            roundtrip(bytes(rng.integers(97, 123, n).astype(np.uint8)))

    def test_fixed_huffman_blocks(self):
        # tiny compressible payloads make zlib pick FIXED codes
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = c.compress(b"hellohellohello") + c.flush()
        out = _native.host_inflate_segment(raw, 15)
        assert out == b"hellohellohello"

    def test_malformed_streams_error_not_hang(self):
        rng = np.random.default_rng(3)
        data = bytes(rng.integers(65, 90, 200_000).astype(np.uint8))
        gz = P.compress_bytes(data, "gzip")
        body_off, segs, _, _ = P.parse_gz_segments(gz)
        c0, u0 = segs[0]
        seg = bytearray(gz[body_off:body_off + c0])
        for trial in range(60):
            bad = bytearray(seg)
            flips = rng.integers(0, len(bad), 3)
            for f in flips:
                bad[int(f)] ^= 1 << int(rng.integers(0, 8))
            try:
                out = _native.host_inflate_segment(bytes(bad), u0)
                # a flip may land in padding/ignored bits: output must
                # still be the exact expected length if it "succeeds"
                assert len(out) == u0
            except RuntimeError as e:
                assert "cause" in str(e)

    def test_truncated_stream_errors(self):
        data = b"x" * 50_000
        gz = P.compress_bytes(data, "gzip")
        body_off, segs, _, _ = P.parse_gz_segments(gz)
        c0, u0 = segs[0]
        seg = gz[body_off:body_off + c0]
        with pytest.raises(RuntimeError):
            _native.host_inflate_segment(seg[: len(seg) // 2], u0)

    @pytest.mark.parametrize("seed", range(5))
    def test_mixed_entropy_fuzz(self, seed):
        rng = np.random.default_rng(100 + seed)
        pieces = []
        for _ in range(int(rng.integers(3, 9))):
            n = int(rng.integers(1, 120_000))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                pieces.append(rng.bytes(n))
            elif kind == 1:
                pieces.append(bytes(rng.integers(60, 70, n).astype(np.uint8)))
            else:
                pieces.append((b"abc123" * (n // 6 + 1))[:n])
        roundtrip(b"".join(pieces))


class TestRootTableEdges:
    """Root-table decode paths (10-bit lit, 8-bit dist tables with compare-
    chain fallback for longer codes): data shaped to force each regime."""

    def test_long_distance_codes_fallback(self):
        # far-apart repeats at many distances -> wide distance alphabet with
        # codes longer than the 8-bit dist table covers
        rng = np.random.default_rng(7)
        base = rng.bytes(40_000)
        parts = [base]
        for d in (33, 1025, 4097, 16385, 30000, 32767):
            parts.append(base[:200])
            parts.append(rng.bytes(d % 7000 + 100))
        parts.append(base)  # long match at large distance
        roundtrip(b"".join(parts))

    def test_skewed_literal_histogram_long_lit_codes(self):
        # extreme skew gives rare symbols 13-15 bit codes -> lit-table miss
        rng = np.random.default_rng(8)
        counts = np.ones(256, np.int64)
        counts[:4] = 200_000
        data = np.repeat(np.arange(256, dtype=np.uint8), counts)
        rng.shuffle(data[:800_000//2])
        roundtrip(bytes(data.tobytes()))

    def test_match_heavy_dictionary_text(self):
        words = [b"alpha", b"bravo", b"charlie", b"delta", b"echo", b"tfrec"]
        rng = np.random.default_rng(9)
        data = b" ".join(words[int(i)] for i in rng.integers(0, 6, 300_000))
        roundtrip(data)

    @pytest.mark.parametrize("seed", range(4))
    def test_bitflip_fuzz_tables(self, seed):
        """Corrupted streams must error, never hang or mis-decode silently
        through the table fast path."""
        rng = np.random.default_rng(100 + seed)
        data = b" ".join(
            [b"token%d" % i for i in rng.integers(0, 50, 20_000)])
        gz = P.compress_bytes(data, "gzip")
        meta = P.parse_gz_segments(gz)
        body_off, segs, crc, isize = meta
        c0, u0 = segs[0]
        seg = bytearray(gz[body_off:body_off + c0])
        for _ in range(60):
            i = int(rng.integers(0, len(seg)))
            bit = 1 << int(rng.integers(0, 8))
            seg[i] ^= bit
            try:
                out = _native.host_inflate_segment(bytes(seg), u0)
                # a flip may legitimately decode to different bytes; the
                # gzip layer catches that via CRC32. Here we only require
                # no hang/crash and correct length.
                assert len(out) == u0
            except RuntimeError:
                pass
            seg[i] ^= bit


WIDTHS = [(10, 8), (9, 7)]  # whole-/half-wave kernels, quarter-wave kernel
VALID = C.valid_segments()
MALFORMED = C.malformed_segments()


class TestHandBuiltSegments:
    """tests/inflate_cases.py through the host build of the core, at the
    root-table widths of every device instantiation: the serial half of
    what tests/test_gpu_inflate.py asks of the kernels."""

    @pytest.mark.parametrize("lit_bits,dist_bits", WIDTHS)
    def test_valid_segments_match_zlib(self, lit_bits, dist_bits):
        for name, comp, want in VALID:
            got = _native.host_inflate_segment(comp, len(want), lit_bits,
                                               dist_bits)
            assert got == want, name

    def test_default_widths_are_10_and_8(self):
        name, comp, want = VALID[0]
        assert _native.host_inflate_segment(comp, len(want)) == want
        with pytest.raises(ValueError):
            _native.host_inflate_segment(comp, len(want), 11, 8)

    def test_long_code_block_misses_the_root_tables(self):
        """The case set's long-code block has lit/len and distance codes of
        every length 1..15, so both table widths fall through to the compare
        chain, and the 10-bit literal and 8-bit distance do so at 9/7 only."""
        assert sorted(C.LONG_LIT.values()) == list(range(1, 16)) + [15]
        assert sorted(C.LONG_DIST.values()) == list(range(1, 16)) + [15]
        assert C.LONG_LIT[ord("g")] == 10 and C.LONG_DIST[4] == 8
        geo = dict((n, w) for n, _, w in VALID)["long_geometry_final"]
        assert b"g" in geo and b"\xff" in geo and len(geo) > 40_000

    @pytest.mark.parametrize("name,comp,expect,cause", MALFORMED,
                             ids=[m[0] for m in MALFORMED])
    def test_malformed_segment_is_refused(self, name, comp, expect, cause):
        got = [C.host_cause(comp, expect, lb, db) for lb, db in WIDTHS]
        assert got[0] != 0 and got[0] == got[1]
        if cause is not None:
            assert got[0] == cause

    def test_every_cause_code_is_reached(self):
        assert {m[3] for m in MALFORMED} >= set(range(1, 18))

    def test_gz_file_helper_writes_the_library_layout(self):
        by_name = {n: (c, w) for n, c, w in VALID}
        segs = [by_name["long_geometry_sync"], by_name["fixed_literals_sync"],
                by_name["stored_65535"]]
        gz, data = C.gz_file(segs)
        body_off, table, crc, isize = P.parse_gz_segments(gz)
        assert table == [(len(c), len(w)) for c, w in segs]
        assert isize == len(data) and crc == zlib.crc32(data)
        assert gzip.decompress(gz) == data == P._gunzip_parallel(gz)
        ours = P.compress_bytes(b"", "gzip")
        assert C.gz_file([by_name["empty_as_zlib_writes_it"]])[0] == ours
