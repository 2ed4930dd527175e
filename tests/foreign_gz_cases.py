"""gzip files as other programs write them (no segment table), shared by the
foreign-gzip inflater tests (test_inflate_foreign_core.py on the CPU,
test_gpu_inflate_foreign.py on the GPU). Everything is generated from seeds
with Python's zlib and gzip, which are such other programs."""

import functools
import gzip
import struct
import zlib

import numpy as np

WORDS = [b"feature", b"int64_list", b"bytes_list", b"value", b"float_list",
         b"\x0a\x0b\x0a\x03", b"label", b"\x12\x08", b"tfrecord", b"key"]


def _rand(seed: int, n: int, lo: int = 0, hi: int = 256) -> bytes:
    return bytes(np.random.default_rng(seed).integers(lo, hi, n)
                 .astype(np.uint8))


def wrap(body: bytes, data: bytes, *, fname=None, fcomment=None, fhcrc=False,
         fextra=None) -> bytes:
    """One gzip member around a raw deflate body (RFC 1952)."""
    flg = ((4 if fextra is not None else 0) | (8 if fname is not None else 0) |
           (16 if fcomment is not None else 0) | (2 if fhcrc else 0))
    hdr = b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00" + b"\x00\x03"
    if fextra is not None:
        hdr += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        hdr += fname + b"\x00"
    if fcomment is not None:
        hdr += fcomment + b"\x00"
    if fhcrc:
        hdr += struct.pack("<H", zlib.crc32(hdr) & 0xFFFF)
    return hdr + body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF,
                                    len(data) % (1 << 32))


def raw_deflate(data: bytes, level=6, mem_level=8, flushes=()) -> bytes:
    """Raw deflate of data; flushes = [(offset, zlib flush mode)]."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level)
    out = []
    pos = 0
    for off, mode in flushes:
        out.append(c.compress(data[pos:off]))
        out.append(c.flush(mode))
        pos = off
    out.append(c.compress(data[pos:]))
    out.append(c.flush())
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def text400k() -> bytes:
    return _rand(0, 400_000, 65, 75)


@functools.lru_cache(maxsize=None)
def fixed_mix_data() -> bytes:
    rng = np.random.default_rng(11)
    idx = rng.integers(0, 14, 150_000)
    rnd = rng.integers(0, 256, idx.size)
    return b"".join(WORDS[i] if i < 10 else bytes([rnd[k]])
                    for k, i in enumerate(idx.tolist()))


@functools.lru_cache(maxsize=None)
def main_cases():
    """[(name, gzip bytes, data, chunk stride, live-chunk condition)] — the
    condition is ('min', n) or ('eq', n) on stats['live_chunks']."""
    t = text400k()
    fm = fixed_mix_data()
    st = _rand(1, 200_000)
    return [
        ("dyn_small_blocks", wrap(raw_deflate(t, 6, 1), t), t, 2048,
         ("min", 50)),
        ("dyn_default", gzip.compress(t, 6), t, 16 << 10, ("min", 4)),
        ("fixed_mix", wrap(raw_deflate(fm, 6, 2), fm), fm, 4096, ("min", 2)),
        ("stored", gzip.compress(st, 6), st, 4096, ("eq", 1)),
    ]


SMALL = _rand(2, 3000, 97, 110)


@functools.lru_cache(maxsize=None)
def variant_cases():
    """[(name, gzip bytes, data, chunk stride)]: header variants and edges,
    all of which the inflater must accept."""
    body = raw_deflate(SMALL)
    block = _rand(7, 40_000)
    far = block + block
    t = text400k()[:150_000]
    return [
        ("hdr_all", wrap(body, SMALL, fname=b"part-00000.tfrecord",
                         fcomment=b"written elsewhere", fhcrc=True,
                         fextra=b"XY\x03\x00abc"), SMALL, 1024),
        ("hdr_fextra_no_ts", wrap(body, SMALL, fextra=b"AB\x02\x00zz"), SMALL,
         1024),
        ("one_byte", gzip.compress(b"x"), b"x", 1024),
        # the repeat lies 40000 back, beyond the window: no match may use it
        ("far_repeat", wrap(raw_deflate(far, 6, 1), far), far, 1024),
        ("window_edge", *window_edge_case(), 1024),
        ("sync_flush", wrap(raw_deflate(t, 6, 8, [(70_000, zlib.Z_SYNC_FLUSH)]),
                            t), t, 4096),
        ("full_flush", wrap(raw_deflate(t, 6, 8, [(70_000, zlib.Z_FULL_FLUSH)]),
                            t), t, 4096),
    ]


def window_edge_case():
    """Text whose second half repeats the first at zlib's farthest reach
    (32768 - 262), so matches cross chunk boundaries at full distance."""
    block = _rand(9, 32768 - 262, 97, 123)
    data = block + block
    return wrap(raw_deflate(data, 9, 1), data), data


@functools.lru_cache(maxsize=None)
def rejected_cases():
    """[(name, gzip bytes, host zlib result or None)]: files the speculative
    path must refuse. The last column is what the host path makes of the
    file: its bytes, or None where it raises too."""
    t = text400k()[:120_000]
    gz = wrap(raw_deflate(t, 6, 1), t)
    two = gz + wrap(raw_deflate(SMALL), SMALL)
    bad_crc = bytearray(gz)
    bad_crc[-8] ^= 0x01
    bad_isize = bytearray(gz)
    bad_isize[-4] ^= 0x01
    flipped = bytearray(gz)
    flipped[10 + (len(gz) - 18) // 2] ^= 0x10
    return [
        ("two_members", two, t + SMALL),
        ("truncated", gz[:len(gz) // 2] + gz[-8:], None),
        ("bad_crc", bytes(bad_crc), None),
        ("bad_isize", bytes(bad_isize), None),
        ("bit_flip", bytes(flipped), None),
    ]


EMPTY = gzip.compress(b"")
