"""Shared cases for the Snappy compressor tests (no tests here): inputs as
(name, data, block), the smallest that reach each branch of
csrc/snappy_enc_core.h, a parser that turns a raw chunk into its elements,
and the container image assembled on the host from the host build of the
core."""

import struct

import numpy as np

from snappy_cases import example_image, varint

BLOCK = 64 << 10


def _rand(seed, n, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n).astype(
        np.uint8).tobytes()


def _other(b: int) -> bytes:
    """One byte that differs from b."""
    return bytes([(b + 1) & 0xFF])


def _bucket(four: bytes) -> int:
    """The core's hash of four bytes (csrc/snappy_enc_core.h)."""
    v = int.from_bytes(four, "little")
    return ((v * 0x9E3779B1) & 0xFFFFFFFF) >> 20


def _found_at_start(data: bytes, copies, upto: int) -> bool:
    """The table keeps one position per bucket, the latest. True when no
    position below `upto` other than `copies` shares the bucket of the
    repeated string's first four bytes, so that a repeat is found at its
    first byte, not a few bytes in."""
    b = _bucket(data[copies[0]:copies[0] + 4])
    return all(_bucket(data[p:p + 4]) != b
               for p in range(upto) if p not in copies)


def repeat_case(length, dist, seed, tail=37):
    """`length` random bytes, random filler, the same bytes again `dist`
    after their first copy, then a random tail. The bytes behind the two
    copies differ, so the repeat is exactly `length` long."""
    while True:
        s = _rand(seed, length)
        fill = _rand(seed + 1, dist - length)
        rest = _rand(seed + 2, tail)
        if fill:
            rest = _other(fill[0]) + rest[1:]
        data = s + fill + s + rest
        if _found_at_start(data, (0,), dist):
            return data
        seed += 1000


def gap_case(gap, seed):
    """Two repeats of a 20-byte string with `gap` random bytes between
    them: the literal between the two copies is exactly `gap` long."""
    while True:
        s = _rand(seed, 20)
        f1 = _rand(seed + 1, 70)
        g = _rand(seed + 2, gap)
        g = _other(f1[0]) + g[1:]  # the first repeat ends where the gap starts
        data = s + f1 + s + g + s + _other(g[0]) + _rand(seed + 3, 30)
        if _found_at_start(data, (0, 90), 110 + gap):
            return data
        seed += 1000


def literal_hdr_len(n: int) -> int:
    """Bytes of the minimal literal header for n >= 1 bytes."""
    n -= 1
    return 1 if n < 60 else 1 + (n.bit_length() + 7) // 8


def one_literal_len(n: int) -> int:
    return len(varint(n)) + (literal_hdr_len(n) + n if n else 0)


def cases():
    """[(name, data, block)]; len(data) == 0 only in the first one."""
    r100 = _rand(40, 100)
    r200 = _rand(41, 200)
    out = [("empty", b"", BLOCK)]
    for n in (1, 3, 4, 63, 64, 65):
        out.append((f"random_{n}", _rand(n, n), BLOCK))
    out += [
        ("abcd_x5000", b"abcd" * 5000, BLOCK),
        ("zeros_70000", bytes(70000), BLOCK),
        ("random_64k", _rand(2, BLOCK), BLOCK),
        ("letters_64k", _rand(3, BLOCK, 97, 123), BLOCK),
        ("example_200_rows", example_image(200), BLOCK),
        # the repeat starts at byte 100 and runs over the window edge at 128
        ("match_crosses_window", r100 + r100[:80] + _rand(42, 20), BLOCK),
        ("match_ends_at_block_end", r200 + r200[:50], BLOCK),
    ]
    for length in (11, 12):
        for dist in (2047, 2048):
            out.append((f"repeat_{length}_at_{dist}",
                        repeat_case(length, dist, 50 + length + dist), BLOCK))
    for length in (64, 65, 67, 68):
        out.append((f"repeat_{length}_split",
                    repeat_case(length, length + 100, 60 + length), BLOCK))
    for gap in (60, 61, 256, 257):
        out.append((f"literal_{gap}_between_matches", gap_case(gap, 70 + gap),
                    BLOCK))
    # the 3-byte copy saves one byte, the second literal's header costs
    # three: the elements lose to the single literal
    out.append(("fallback_after_copy", repeat_case(4, 2504, 90, tail=2496),
                BLOCK))
    far = _rand(80, 65537)
    out.append(("repeat_beyond_65535_in_128k", far + far[:60000], 128 << 10))
    out.append(("block_1000", example_image(200)[:5300], 1000))
    return out


def blocks(data: bytes, block: int):
    return [data[p:p + block] for p in range(0, len(data), block)]


def elements(chunk: bytes, n: int):
    """[(kind, len, offset)] of a raw chunk of n uncompressed bytes: kind 0
    is a literal (offset 0), kinds 1..3 the copy tags. Checks the framing
    (preamble, every element inside the chunk, lengths adding up to n)."""
    pre = varint(n)
    assert chunk[:len(pre)] == pre
    pos = len(pre)
    out = []
    produced = 0
    while pos < len(chunk):
        tag = chunk[pos] & 3
        up6 = chunk[pos] >> 2
        if tag == 0:
            hdr = 1
            length = up6 + 1
            if up6 >= 60:
                nb = up6 - 59
                hdr = 1 + nb
                length = int.from_bytes(chunk[pos + 1:pos + 1 + nb],
                                        "little") + 1
            assert literal_hdr_len(length) == hdr, "literal header not minimal"
            pos += hdr + length
            out.append((0, length, 0))
        elif tag == 1:
            length = 4 + (up6 & 7)
            out.append((1, length, ((up6 >> 3) << 8) | chunk[pos + 1]))
            pos += 2
        elif tag == 2:
            length = up6 + 1
            out.append((2, length,
                        int.from_bytes(chunk[pos + 1:pos + 3], "little")))
            pos += 3
        else:
            length = up6 + 1
            out.append((3, length,
                        int.from_bytes(chunk[pos + 1:pos + 5], "little")))
            pos += 5
        assert pos <= len(chunk)
        produced += length
    assert produced == n
    return out


def host_chunk(raw: bytes) -> bytes:
    from spark_tfrecord_amd import _native

    return bytes(_native.host_snap_chunk(raw))


def host_snappy_image(data: bytes, block: int) -> bytes:
    """The `.snappy` file image of `data`, one chunk per block, from the
    host build of the compressor core."""
    return b"".join(
        struct.pack(">II", len(raw), len(c)) + c
        for raw, c in ((raw, host_chunk(raw)) for raw in blocks(data, block)))
