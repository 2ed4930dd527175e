"""Shared cases for the Snappy tests (no tests here): raw chunks as
(name, comp_bytes, expected_bytes), malformed chunks as (name, comp_bytes,
expect_len, cause), and Hadoop-framed file images built with struct around
them. The layout is the one io/paths.py snappy_walk describes; the hand-
assembled chunks cover encodings the library never emits."""

import struct

import numpy as np
import pyarrow as pa

from spark_tfrecord_amd.io import paths as P

_CODEC = pa.Codec("snappy")

# cause codes of csrc/snappy_core.h
(SN_PREAMBLE_LONG, SN_PREAMBLE_MISMATCH, SN_OFFSET_ZERO, SN_OFFSET_FAR,
 SN_OPERAND_PAST_INPUT, SN_LITERAL_PAST_INPUT, SN_OUTPUT_OVERRUN,
 SN_INPUT_SHORT, SN_INPUT_LEFT) = range(1, 10)


def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def lit_element(data: bytes, form: int = None) -> bytes:
    """Literal element; `form` = number of length bytes (0 = inline, only
    for 1..60), default the minimal one."""
    n = len(data) - 1
    if form is None:
        form = 0 if n < 60 else (n.bit_length() + 7) // 8
    if form == 0:
        assert n < 60
        return bytes([n << 2]) + data
    assert n < (1 << (8 * form))
    return bytes([(59 + form) << 2]) + n.to_bytes(form, "little") + data


def copy_element(tag: int, length: int, offset: int) -> bytes:
    if tag == 1:
        assert 4 <= length <= 11 and 0 <= offset < 2048
        return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5),
                      offset & 0xFF])
    assert 1 <= length <= 64
    if tag == 2:
        return bytes([2 | ((length - 1) << 2)]) + offset.to_bytes(2, "little")
    return bytes([3 | ((length - 1) << 2)]) + offset.to_bytes(4, "little")


class Chunk:
    """Assembles a raw chunk element by element and plays it forward, so
    the expected bytes come from the definition of the elements alone."""

    def __init__(self):
        self.body = bytearray()
        self.out = bytearray()
        self.elements = []  # each element's bytes, in order

    def lit(self, data: bytes, form: int = None):
        e = lit_element(data, form)
        self.body += e
        self.elements.append(e)
        self.out += data
        return self

    def copy(self, tag: int, length: int, offset: int):
        assert 0 < offset <= len(self.out)
        e = copy_element(tag, length, offset)
        self.body += e
        self.elements.append(e)
        for _ in range(length):
            self.out.append(self.out[-offset])
        return self

    def comp(self) -> bytes:
        return varint(len(self.out)) + bytes(self.body)

    def case(self, name):
        return (name, self.comp(), bytes(self.out))


def _rand(n, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n).astype(
        np.uint8).tobytes()


def example_image(rows=200) -> bytes:
    from bench import make_batch
    from spark_tfrecord_amd.engine import cpu as cpu_engine

    return bytes(cpu_engine.encode_batch(make_batch(rows, seed=3), "Example"))


def library_chunks():
    datas = [
        ("empty", b""),
        ("one_byte", b"\x2a"),
        ("random_100", _rand(100, 1)),
        ("abcd_x5000", b"abcd" * 5000),
        ("zeros_70000", bytes(70000)),
        ("letters_64k", _rand(64 << 10, 2, 97, 123)),
        ("example_200_rows", example_image(200)),
    ]
    return [(n, _CODEC.compress(d, asbytes=True), d) for n, d in datas]


def hand_chunks():
    cases = []
    for n in (60, 61, 256, 257):
        cases.append(Chunk().lit(_rand(n, n)).case(f"literal_{n}"))
    for form in (2, 3, 4):
        cases.append(Chunk().lit(b"hello", form)
                     .case(f"literal_5_in_{form}_byte_form"))
    c = Chunk().lit(_rand(2047, 10))
    for length in (4, 11):
        for off in (1, 2047):
            c.copy(1, length, off)
    cases.append(c.case("copy01_len_4_11_off_1_2047"))
    c = Chunk().lit(_rand(65535, 11))
    for length in (1, 64):
        for off in (1, 3, 63, 64, 65535):
            c.copy(2, length, off)
    cases.append(c.case("copy10_len_1_64_offsets"))
    c = Chunk().lit(_rand(40, 12)).copy(3, 30, 5).copy(3, 64, 5).copy(3, 1, 5)
    cases.append(c.case("copy11_off_5"))
    c = Chunk().lit(_rand(70000, 13)).copy(3, 64, 70000).copy(3, 7, 70000)
    c.lit(_rand((128 << 10) - len(c.out) - 64, 14)).copy(3, 64, 70000)
    assert len(c.out) == 128 << 10
    cases.append(c.case("copy11_off_70000_in_128k"))
    cases.append(Chunk().lit(b"0123456789").copy(2, 10, 10)
                 .case("copy_source_at_byte_0"))
    cases.append(Chunk().lit(b"xyz").copy(1, 11, 2)
                 .case("copy_ends_at_expect_len"))
    # 200 four-byte elements (3-byte literals) back to back. Starts advance
    # by 4, so a leading literal of 1..4 bytes shifts the phase: over the
    # four chunks the starts fall on every residue mod 64.
    for shift in range(4):
        c = Chunk().lit(_rand(shift + 1, 20 + shift))
        for k in range(200):
            c.lit(bytes([k & 0xFF, shift, 0x5A]))
        cases.append(c.case(f"elements_4_bytes_x200_shift_{shift}"))
    return cases


def valid_chunks():
    return library_chunks() + hand_chunks()


def malformed_chunks():
    """One chunk per refusal of the core, each one edit away from the valid
    chunk `base`: (name, comp, expect_len, cause)."""
    base = Chunk().lit(b"snappy-chunk-").copy(2, 20, 7).lit(b"tail").copy(
        2, 9, 3)
    n = len(base.out)
    pre = varint(n)
    body = bytes(base.body)
    elems = base.elements
    assert len(pre) == 1 and b"".join(elems) == body
    lit_last = Chunk().lit(b"snappy-chunk-").copy(2, 20, 7).lit(b"tail")
    out = [
        ("preamble_6_bytes", b"\x80" * 5 + b"\x00" + body, n,
         SN_PREAMBLE_LONG),
        ("preamble_off_by_one", varint(n + 1) + body, n,
         SN_PREAMBLE_MISMATCH),
        ("offset_zero", pre + elems[0] + copy_element(2, 20, 0) + elems[2]
         + elems[3], n, SN_OFFSET_ZERO),
        ("offset_past_start", pre + elems[0] + copy_element(2, 20, 14)
         + elems[2] + elems[3], n, SN_OFFSET_FAR),
        ("operand_cut", pre + body[:-1], n, SN_OPERAND_PAST_INPUT),
        ("literal_cut", lit_last.comp()[:-1], len(lit_last.out),
         SN_LITERAL_PAST_INPUT),
        ("output_overrun", pre + b"".join(elems[:3])
         + copy_element(2, 10, 3), n, SN_OUTPUT_OVERRUN),
        ("input_short", pre + b"".join(elems[:3]), n, SN_INPUT_SHORT),
        ("input_left_over", pre + body + lit_element(b"!"), n,
         SN_INPUT_LEFT),
    ]
    assert sorted(c[3] for c in out) == list(range(1, 10))
    return out


# ---------------------------------------------------------------------------
# file images
# ---------------------------------------------------------------------------

def block(chunks) -> bytes:
    """One container block around [(comp, expected), ...]."""
    raw_len = sum(len(e) for _, e in chunks)
    return struct.pack(">I", raw_len) + b"".join(
        struct.pack(">I", len(c)) + c for c, _ in chunks)


def one_chunk_file(comp: bytes, expected: bytes) -> bytes:
    """A file of one block holding `comp` as its one chunk; the empty chunk
    becomes the zero-byte file (a block of raw_len 0 would end the stream)."""
    return block([(comp, expected)]) if expected else b""


def valid_files():
    """(name, file image, expected bytes)."""
    lib = {n: (c, e) for n, c, e in library_chunks()}
    hand = {n: (c, e) for n, c, e in hand_chunks()}
    three = [lib["random_100"], hand["copy10_len_1_64_offsets"],
             lib["abcd_x5000"]]
    files = [
        ("one_block_one_chunk", block([lib["example_200_rows"]]),
         lib["example_200_rows"][1]),
        ("one_block_three_chunks", block(three),
         b"".join(e for _, e in three)),
    ]
    for n in (1, 65535, 65536, 65537):
        d = _rand(n, 30 + n % 7, 97, 105)
        files.append((f"writer_{n}", P.compress_bytes(d, "snappy"), d))
    big = (example_image(200) * 8)[:256 << 10]
    assert len(big) == 256 << 10
    files.append(("block_256k", block([(_CODEC.compress(big, asbytes=True),
                                        big)]), big))
    files.append(("zero_block_at_end",
                  block([lib["random_100"]]) + struct.pack(">I", 0),
                  lib["random_100"][1]))
    return files


def malformed_files():
    """(name, file image): the header walk itself fails."""
    good = block([(c, e) for _, c, e in library_chunks()[1:3]])
    comp, exp = library_chunks()[3][1:]
    return [
        ("cut_in_block_header", good + b"\x00\x00"),
        ("cut_in_chunk_header", good + struct.pack(">I", 5) + b"\x00"),
        ("comp_len_past_eof", good + struct.pack(">II", len(exp),
                                                 len(comp) + 1) + comp),
    ]
