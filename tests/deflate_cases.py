"""Inputs and the host-side reference image shared by the DEFLATE
compressor tests (test_deflate_core.py on the CPU, test_gpu_deflate.py on
the GPU). Every input is the smallest that reaches its branch of
csrc/deflate_core.h."""

import struct
import zlib

import numpy as np

from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P

SEG = 32 << 10  # the default TFREC_GZ_SEGMENT, passed explicitly


def seg_out_bound(u: int) -> int:
    return u + 5 * (-(-u // 65535)) + 5


def _rand(seed: int, n: int, lo: int = 0, hi: int = 256) -> bytes:
    return bytes(np.random.default_rng(seed).integers(lo, hi, n)
                 .astype(np.uint8))


def _de_bruijn(k: int, n: int) -> bytes:
    """Cyclic sequence over k symbols in which every n-gram occurs once:
    no 3-byte match exists anywhere in its linear prefix."""
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return bytes(65 + s for s in seq)


def cases():
    """[(name, data, segment size)]"""
    text = _rand(25, 2 * 4096 + 7, 97, 122)  # 25-symbol "text"
    block = _rand(7, 40000)
    out = [(f"len{n}", b"abcd"[:n], SEG) for n in range(5)]
    out += [
        ("run258", b"r" * 258, SEG),
        ("run259", b"r" * 259, SEG),
        ("same32k", b"\x00" * 32768, SEG),
        ("pattern64", _rand(3, 64) * 512, SEG),
        ("alpha2", _rand(2, 32768, 0, 2), SEG),
        ("alpha4", _rand(4, 32768, 0, 4), SEG),
        ("alpha25", _rand(5, 32768, 97, 122), SEG),      # dynamic codes
        ("random128k", _rand(6, 128 << 10), 128 << 10),  # several stored blocks
        ("seg-1", text[:4095], 4096),
        ("seg", text[:4096], 4096),
        ("seg+1", text[:4097], 4096),   # final segment of one byte
        ("2seg+7", text, 4096),
        ("far_repeat", block + block, 96 << 10),  # repeats only beyond 32768
        ("distinct256", bytes(range(256)), SEG),  # no match at all
        ("one_distance", _rand(8, 100) * 40, SEG),
        ("no_trigram_repeat", _de_bruijn(8, 3), SEG),  # dynamic, no distances
        ("one_literal", b"a" * 64, SEG),  # one literal + EOB, no distances
    ]
    return out


def split(data: bytes, seg: int):
    """compress_bytes' segmentation: at least one (possibly empty) segment."""
    n = len(data)
    return [data[lo:lo + seg] for lo in range(0, max(n, 1), seg)]


def host_segments(data: bytes, seg: int, threshold=None):
    if threshold is None:
        threshold = P._GZ_STORED_THRESHOLD
    parts = split(data, seg)
    return [_native.host_deflate_segment(p, i == len(parts) - 1, threshold)
            for i, p in enumerate(parts)]


def host_gzip_image(data: bytes, seg: int, threshold=None) -> bytes:
    """Whole gzip file from host-core segments, in compress_bytes' header
    format; CRC-32 and ISIZE come from zlib, not from the code under test."""
    parts = split(data, seg)
    bodies = host_segments(data, seg, threshold)
    payload = struct.pack("<BBH", 1, 0, len(parts)) + b"".join(
        struct.pack("<II", len(b), len(p)) for b, p in zip(bodies, parts))
    extra = b"TS" + struct.pack("<H", len(payload)) + payload
    hdr = (b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" +
           struct.pack("<H", len(extra)) + extra)
    trailer = struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF,
                          len(data) % (1 << 32))
    return hdr + b"".join(bodies) + trailer
