"""Raw-deflate segments for the segmented-gzip inflater (csrc/inflate_core.h,
csrc/hip/inflate.hip), shared by test_inflate_core.py on the CPU and
test_gpu_inflate.py on the GPU. Most are assembled bit by bit here, so that
code lengths, match geometry and block alignment are chosen and not left to
a compressor; `zlib.decompressobj(-15)` is the only reference, and every
case is checked against it when this module is imported."""

import functools
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43,
            51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4,
             4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257,
             385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9,
              9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
SYNC = b"\x00\x00\xff\xff"


class BitWriter:
    """LSB-first bit packer (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def clone(self):
        w = BitWriter()
        w.out, w.acc, w.n = bytearray(self.out), self.acc, self.n
        return w

    def bits(self, value, k):
        self.acc |= (value & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code_len):
        """A Huffman code goes in most significant bit first."""
        code, k = code_len
        rev = 0
        for _ in range(k):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.bits(rev, k)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def bit_length(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        w = self.clone()
        w.align()
        return bytes(w.out)


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code (RFC 1951 3.2.2) for
    a list of code lengths indexed by symbol; 0 = symbol unused."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * 16
    code = 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)
# the code-length code every dynamic header here uses: complete, 13/16 +
# 6/32, all 19 symbols present
CL_LENS = [4] * 13 + [5] * 6
CL_CODE = canonical(CL_LENS)


def lens_of(pairs, n):
    """Length list of n symbols from {symbol: length}."""
    out = [0] * n
    for s, l in pairs.items():
        out[s] = l
    return out


class Stream:
    """One raw-deflate segment, assembled block by block and played forward
    (self.data is what a decoder must produce)."""

    def __init__(self):
        self.w = BitWriter()
        self.data = bytearray()
        self.lit_code = self.dist_code = None

    def clone(self):
        s = Stream()
        s.w, s.data = self.w.clone(), bytearray(self.data)
        s.lit_code, s.dist_code = self.lit_code, self.dist_code
        return s

    def stored(self, payload, final=False):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(0, 2)
        self.w.align()
        n = len(payload)
        self.w.raw(struct.pack("<HH", n, n ^ 0xFFFF) + payload)
        self.data += payload
        return self

    def fixed(self, final=False):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self.lit_code, self.dist_code = FIXED_LIT, FIXED_DIST
        return self

    def dynamic(self, lit_lens, dist_lens, final=False, use_repeats=True):
        """Header of a dynamic block with these code lengths (lists indexed
        by symbol, at least 257 and 1 long)."""
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        w.bits(len(lit_lens) - 257, 5)
        w.bits(len(dist_lens) - 1, 5)
        w.bits(19 - 4, 4)
        for s in CL_ORDER:
            w.bits(CL_LENS[s], 3)
        seq = list(lit_lens) + list(dist_lens)
        i = 0
        while i < len(seq):
            v = seq[i]
            run = 1
            while i + run < len(seq) and seq[i + run] == v:
                run += 1
            if use_repeats and v == 0 and run >= 3:
                take = min(run, 138)
                if take >= 11:
                    w.code(CL_CODE[18])
                    w.bits(take - 11, 7)
                else:
                    w.code(CL_CODE[17])
                    w.bits(take - 3, 3)
                i += take
            elif use_repeats and v and run >= 4:
                take = min(run - 1, 6)
                w.code(CL_CODE[v])
                w.code(CL_CODE[16])
                w.bits(take - 3, 2)
                i += 1 + take
            else:
                w.code(CL_CODE[v])
                i += 1
        self.lit_code = canonical(lit_lens)
        self.dist_code = canonical(dist_lens)
        return self

    def lit(self, *values):
        for v in values:
            self.w.code(self.lit_code[v])
            self.data.append(v)
        return self

    def lits(self, payload):
        return self.lit(*payload)

    def match(self, length, dist, len_sym=None, play=True):
        ls = len_sym if len_sym is not None else max(
            i for i in range(29) if LEN_BASE[i] <= length)
        self.w.code(self.lit_code[257 + ls])
        self.w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.w.code(self.dist_code[ds])
        self.w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])
        if play:
            assert dist <= len(self.data)
            for _ in range(length):
                self.data.append(self.data[-dist])
        return self

    def end(self):
        self.w.code(self.lit_code[256])
        return self

    def sync(self):
        """The empty stored block a Z_FULL_FLUSH closes a segment with."""
        return self.stored(b"")

    def comp(self):
        return self.w.getvalue()

    def case(self, name):
        return (name, self.comp(), bytes(self.data))


def zlib_inflate(comp):
    """(bytes, reached the final block) as zlib decodes a raw segment."""
    d = zlib.decompressobj(-15)
    out = d.decompress(comp) + d.flush()
    return out, d.eof


def zlib_refuses(comp, expect):
    try:
        return len(zlib_inflate(comp)[0]) != expect
    except zlib.error:
        return True


def is_final(comp):
    return zlib_inflate(comp)[1]


def _rand(seed, n, lo=0, hi=256):
    return bytes(np.random.default_rng(seed).integers(lo, hi, n)
                 .astype(np.uint8))


# ---------------------------------------------------------------------------
# the long-code block: lit/len lengths 1..15,15 and distance lengths
# 1..15,15, so codes of every length occur, those beyond the 10/8-bit and
# 9/7-bit root tables included (a 10-bit literal and an 8-bit distance hit
# the wide tables and miss the narrow ones)
# ---------------------------------------------------------------------------

LONG_LIT = {ord("a"): 1, ord("b"): 2, ord("c"): 3, 257: 4, ord("d"): 5,
            264: 6, ord("e"): 7, 285: 8, ord("f"): 9, ord("g"): 10,
            ord("h"): 11, 265: 12, 256: 13, ord("i"): 14, 0xFF: 15, 284: 15}
LONG_DIST = {0: 1, 6: 2, 1: 3, 16: 4, 2: 5, 29: 6, 3: 7, 4: 8, 5: 9, 28: 10,
             10: 11, 13: 12, 20: 13, 22: 14, 25: 15, 27: 15}
LONG_LIT_LENS = lens_of(LONG_LIT, 286)
LONG_DIST_LENS = lens_of(LONG_DIST, 30)
_LONG_BYTES = b"abcdefghi\xff"
_LONG_WEIGHTS = [.5, .2, .1, .06, .04, .03, .03, .02, .01, .01]

GEOMETRY = [(3, 1), (258, 1), (3, 2), (3, 3), (3, 4), (10, 5), (10, 7),
            (10, 8), (10, 9), (10, 10), (258, 257), (258, 258), (258, 32768),
            (3, 24577), (10, 16385)]
# the other distance codes of the block, and lengths with extra bits
GEOMETRY_MORE = [(11, 33), (12, 48), (250, 97), (257, 128), (3, 1025),
                 (10, 1536), (258, 2049), (12, 3072), (227, 6145), (10, 8192),
                 (11, 12289), (258, 16384), (10, 6), (3, 12), (258, 384)]


def _skewed(seed, n):
    idx = np.random.default_rng(seed).choice(len(_LONG_BYTES), n,
                                             p=_LONG_WEIGHTS)
    return bytes(_LONG_BYTES[i] for i in idx.tolist())


@functools.lru_cache(maxsize=None)
def _long_prefix(nlit):
    """A non-final long-code block opened and `nlit` skewed literals in."""
    s = Stream().dynamic(LONG_LIT_LENS, LONG_DIST_LENS)
    return s.lits(_skewed(40, nlit))


def long_block(nlit=40_000):
    return _long_prefix(nlit).clone()


def _finish(s, final):
    """Close the open block; a non-final segment ends on the sync block."""
    s.end()
    if final:
        # the block was opened non-final: a final empty stored block ends it
        return s.stored(b"", final=True)
    return s.sync()


def _long_cases():
    out = []
    geo = long_block()
    for ln, d in GEOMETRY:          # each match directly after the last
        geo.match(ln, d)
    for k, (ln, d) in enumerate(GEOMETRY + GEOMETRY_MORE):
        # 1..9 literals pending in the 8-byte window when the match comes
        geo.lits(_skewed(100 + k, 1 + k % 9)).match(ln, d)
    geo.match(258, 1, len_sym=27)   # length 258 spelled 227 + 31
    for final in (True, False):
        out.append(_finish(geo.clone(), final).case(
            f"long_geometry_{'final' if final else 'sync'}"))
    # tails: 0..9 literals between the last match and end-of-block
    for t in range(10):
        s = geo.clone().lits(_skewed(200 + t, t))
        out.append(_finish(s, t % 2 == 0).case(f"long_tail_{t}_literals"))
    # near geometry one pair per segment, so a failure names the pair
    for ln, d in GEOMETRY:
        if d > 258:
            continue
        s = long_block(300)
        s.match(ln, d).lits(_skewed(300 + ln + d, 5)).match(ln, d)
        out.append(_finish(s, (ln + d) % 2 == 0).case(f"long_len{ln}_dist{d}"))
    for ln, d in GEOMETRY:
        if d <= 258:
            continue
        s = long_block().match(ln, d).lit(ord("a")).match(ln, d)
        out.append(_finish(s, True).case(f"long_len{ln}_dist{d}"))
    # the literal-only use of every literal code length
    out.append(_finish(long_block(3000), True).case("long_literals_only"))
    return out


SIMPLE_LIT = lens_of({ord("x"): 1, ord("y"): 2, 256: 3, 258: 4, 285: 4}, 286)


def _ending_cases():
    out = []
    text = _rand(50, 400, 97, 101)
    for final in (True, False):
        s = Stream().fixed()
        s.lits(text[:200]).match(30, 200).match(258, 1).lits(text[200:260])
        s.end()
        s.dynamic(LONG_LIT_LENS, LONG_DIST_LENS).lits(_skewed(51, 150))
        s.match(258, 257).match(10, 5).lits(b"abc").end()   # 5 pending bytes
        s.stored(_rand(52, 100))
        s.dynamic(SIMPLE_LIT,
                  lens_of({0: 2, 5: 2, 12: 2, 16: 3, 18: 4, 19: 4}, 30),
                  final=final)
        # into the fixed block, the stored block, the first dynamic block
        s.match(258, 1000).match(4, 90).match(258, 8).match(258, 300)
        s.match(258, 700).lits(b"xyx").match(4, 1).match(258, 96).end()
        if not final:
            s.sync()
        out.append(s.case(f"blocks_fixed_dyn_stored_dyn_"
                          f"{'final' if final else 'sync'}"))
    # one fixed-code symbol per byte: as literal-heavy as a segment gets
    for final in (True, False):
        s = Stream().fixed(final=final).lits(_rand(53 + final, 6001, 0, 144))
        s.end()
        if not final:
            s.sync()
        out.append(s.case(f"fixed_literals_{'final' if final else 'sync'}"))
    out.append(Stream().fixed(final=True).end().case("end_of_block_only"))
    s = Stream().fixed().lits(b"hello").end().fixed().end()
    out.append(s.dynamic(SIMPLE_LIT, [0], final=True).end().case(
        "end_of_block_only_after_data"))
    comp = zlib.compressobj(6, zlib.DEFLATED, -15).flush()
    out.append(("empty_as_zlib_writes_it", comp, b""))
    out.append(Stream().sync().case("empty_sync_only"))
    return out


def _degenerate_dist_cases():
    out = []
    s = Stream().dynamic(SIMPLE_LIT, [0], final=True)
    out.append(s.lits(b"xyyxxxyxyxxy" * 9).end().case("no_distance_code"))
    s = Stream().dynamic(SIMPLE_LIT, [1], final=True)
    s.lits(b"xy").match(4, 1).lit(ord("x")).match(258, 1).match(4, 1)
    out.append(s.lits(b"yyx").end().case("one_distance_code"))
    return out


STORED_FIRST = [0, 1, 7, 8, 9, 63, 64, 65, 511, 513]
STORED_SECOND = [512, 257, 255, 129, 127, 256, 128, 3, 1000, 0]


def _stored_cases():
    out = []
    for r in range(9):
        # r fixed-coded literals put the stored header at bit 10 + 8r: the
        # payload starts at byte 6 + r, every residue of the 8-byte prefetch
        for k, (a, b) in enumerate(zip(STORED_FIRST, STORED_SECOND)):
            s = Stream().fixed().lits(b"ABCDEFGH"[:r]).end()
            s.stored(_rand(1000 + 10 * r + k, a))
            s.stored(_rand(2000 + 10 * r + k, b), final=(r + k) % 2 == 0)
            if not is_final(s.comp()):
                s.sync()
            out.append(s.case(f"stored_after_{r}_literals_{a}_{b}"))
    out.append(Stream().stored(_rand(60, 65535), final=True).case(
        "stored_65535"))
    s = Stream().stored(_rand(61, 300)).fixed(final=True)
    s.match(258, 300).match(10, 10).lits(b"tail").match(42, 300 + 258 + 14)
    out.append(s.end().case("match_reads_stored_bytes"))
    return out


def cut_like_compress_bytes(data, level, strategy, seg=32 << 10):
    """[(comp, want)]: one deflate stream over `data`, a full flush every
    `seg` bytes, as io/paths.py compress_bytes cuts a file."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out = []
    for pos in range(0, len(data), seg):
        hi = min(pos + seg, len(data))
        body = c.compress(data[pos:hi])
        body += c.flush() if hi == len(data) else c.flush(zlib.Z_FULL_FLUSH)
        out.append((body, data[pos:hi]))
    return out


def _zlib_cases():
    words = [b"feature", b"int64_list", b"value", b"\x0a\x0b\x0a\x03",
             b"label", b"tfrecord", b" ", b"\x12\x08"]
    rng = np.random.default_rng(70)
    text = b"".join(words[i] for i in rng.integers(0, 8, 9000).tolist())
    inputs = {"text": text[:40_000],
              "skewed": _skewed(71, 40_000),
              "random": _rand(72, 40_000),
              # near-uniform over 200 values: Huffman-coded, hardly smaller
              "wide": _rand(73, 40_000, 0, 200)}
    modes = [("level1", 1, zlib.Z_DEFAULT_STRATEGY),
             ("level6", 6, zlib.Z_DEFAULT_STRATEGY),
             ("level9", 9, zlib.Z_DEFAULT_STRATEGY),
             ("fixed", 6, zlib.Z_FIXED),
             ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY),
             ("rle", 6, zlib.Z_RLE)]
    out = []
    for mname, level, strategy in modes:
        for iname, data in inputs.items():
            for k, (comp, want) in enumerate(
                    cut_like_compress_bytes(data, level, strategy)):
                out.append((f"zlib_{mname}_{iname}_seg{k}", comp, want))
    return out


@functools.lru_cache(maxsize=None)
def valid_segments():
    """[(name, comp, want)]: raw-deflate segments the inflater must decode
    to exactly `want`. A segment either ends on a final block or, as all
    but the last segment of a file do, on the empty stored block."""
    cases = (_long_cases() + _ending_cases() + _degenerate_dist_cases() +
             _stored_cases() + _zlib_cases())
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    for name, comp, want in cases:
        got, _ = zlib_inflate(comp)
        assert got == want, name
        assert len(want) <= 66_000, name
    return cases


# ---------------------------------------------------------------------------
# malformed segments
# ---------------------------------------------------------------------------

def _dyn_header(cl_lens, hlit=257, hdist=1):
    """A final dynamic block up to and including the code-length code."""
    w = BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(cl_lens[s], 3)
    return w


def _hand_malformed():
    out = []
    ok = Stream().fixed(final=True).lits(b"abcabc").match(5, 3).lit(33).end()
    want = len(ok.data)
    # 1: the input ends before a block header
    out.append(("no_block_header", b"", 5, 1))
    # 2: LEN and NLEN of a stored block disagree
    out.append(("stored_nlen_mismatch", b"\x01\x05\x00\x00\x00hello", 5, 2))
    # 3: a stored block longer than the input left, or than the output left
    out.append(("stored_past_input", b"\x01\x05\x00\xfa\xffhel", 5, 3))
    out.append(("stored_past_output", b"\x01\x05\x00\xfa\xffhello", 4, 3))
    # 4: block type 3
    out.append(("block_type_3", b"\x07\x00", 1, 4))
    # 5: the input ends inside HLIT/HDIST/HCLEN
    out.append(("dynamic_counts_cut", b"\x05", 1, 5))
    # 6: an over-subscribed code-length code (three codes of one bit)
    w = _dyn_header([1, 1, 1] + [0] * 16)
    w.bits(0, 16)
    out.append(("code_length_code_oversubscribed", w.getvalue(), 1, 6))
    # 7: a code-length symbol that no code stands for (the code is
    # incomplete: one code of one bit, and the stream has the other bit)
    w = _dyn_header([1] + [0] * 18)
    w.bits(0xFFFF, 16)
    out.append(("code_length_symbol_unassigned", w.getvalue(), 1, 7))
    # 8: the input ends inside the extra bits of a repeat (symbol 18 ends
    # at bit 79 and wants 7 more bits; 10 bytes hold one)
    w = _dyn_header(CL_LENS)
    w.code(CL_CODE[18])
    w.bits(127, 7)
    assert w.bit_length() == 86
    out.append(("repeat_extra_bits_cut", w.getvalue()[:10], 1, 8))
    # 9, 10: over-subscribed lit/len and distance codes
    s = Stream().dynamic(lens_of({65: 1, 66: 1, 256: 1}, 257), [0],
                         final=True)
    out.append(("litlen_code_oversubscribed", s.comp() + b"\x00\x00", 1, 9))
    s = Stream().dynamic(SIMPLE_LIT, [1, 1, 1], final=True)
    out.append(("distance_code_oversubscribed", s.comp() + b"\x00\x00", 1,
                10))
    # 11: the input ends inside the block's symbols
    out.append(("symbols_cut", ok.comp()[:4], want, 11))
    # 12: a literal beyond the expected length
    out.append(("literal_past_output", ok.comp(), want - 1, 12))
    # 13: length symbols 286 and 287 exist in the fixed code only
    for sym in (286, 287):
        s = Stream().fixed(final=True).lits(b"abc")
        s.w.code(FIXED_LIT[sym])
        s.w.bits(0, 24)
        out.append((f"length_symbol_{sym}", s.comp(), 10, 13))
    # 14: distance symbols 30 and 31, likewise
    for sym in (30, 31):
        s = Stream().fixed(final=True).lits(b"abc")
        s.w.code(FIXED_LIT[257])
        s.w.code(FIXED_DIST[sym])
        s.w.bits(0, 24)
        out.append((f"distance_symbol_{sym}", s.comp(), 10, 14))
    # 15: the input ends inside a distance's extra bits (bit 23 of 24; the
    # code wants 13)
    s = Stream().fixed(final=True).lit(ord("a")).match(3, 32768, play=False)
    assert s.w.bit_length() == 36
    out.append(("distance_extra_bits_cut", s.comp()[:3], 4, 15))
    # 16: a distance before the start of the segment, a match beyond the
    # expected length
    s = Stream().fixed(final=True).lit(ord("a")).match(3, 2, play=False)
    out.append(("distance_before_start", s.end().comp(), 4, 16))
    s = Stream().fixed(final=True).lits(b"abc").match(10, 3).end()
    out.append(("match_past_output", s.comp(), 12, 16))
    # 17: the final block ends short of the expected length
    out.append(("final_block_ends_short", ok.comp(), want + 1, 17))
    return out


def _truncations():
    """Every cut of two short valid segments that zlib, too, cannot decode
    in full (a cut inside the trailing sync block or the last padding leaves
    all the bytes there; zlib then has all of `expect`, and so may the
    core). cause None: whatever the host core says, but not 0."""
    a = Stream().fixed().lits(b"abcabc").match(20, 3)
    a.end().stored(b"stored!").dynamic(SIMPLE_LIT, [1])
    a.lits(b"xyx").match(4, 1).end().sync()
    b = long_block(60).match(10, 8).match(258, 1).lits(b"abc").end()
    b.stored(b"", final=True)
    out = []
    for tag, s in (("a", a), ("b", b)):
        comp, want = s.comp(), len(s.data)
        assert zlib_inflate(comp)[0] == bytes(s.data)
        for cut in range(len(comp)):
            if zlib_refuses(comp[:cut], want):
                out.append((f"cut_{tag}_at_{cut}", comp[:cut], want, None))
    return out


@functools.lru_cache(maxsize=None)
def malformed_segments():
    """[(name, comp, expect, cause)]: segments the inflater must refuse.
    `cause` is inflate_one's code as the host build returns it (the CPU
    tier checks that), or None for the truncations, whose cause the tests
    take from the host build. Every code 1..17 is reached."""
    cases = _hand_malformed() + _truncations()
    for name, comp, expect, _ in cases:
        assert zlib_refuses(comp, expect), name
    assert {c[3] for c in cases} - {None} == set(range(1, 18))
    return cases


def host_cause(comp, expect, lit_bits=10, dist_bits=8):
    """inflate_one's return code from the host build (0 = accepted)."""
    from spark_tfrecord_amd import _native

    try:
        _native.host_inflate_segment(comp, expect, lit_bits, dist_bits)
    except RuntimeError as e:
        return int(str(e).rsplit("cause ", 1)[1])
    return 0


# ---------------------------------------------------------------------------
# whole files
# ---------------------------------------------------------------------------

def gz_file(segments):
    """A gzip file in the layout io/paths.py compress_bytes writes (FEXTRA
    'TS' table, CRC-32/ISIZE trailer) around [(comp, want)] segments: all
    but the last must end on the sync block, the last on a final block."""
    for k, (comp, _) in enumerate(segments):
        assert is_final(comp) == (k == len(segments) - 1), k
    data = b"".join(w for _, w in segments)
    payload = struct.pack("<BBH", 1, 0, len(segments)) + b"".join(
        struct.pack("<II", len(c), len(w)) for c, w in segments)
    extra = b"TS" + struct.pack("<H", len(payload)) + payload
    hdr = (b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" +
           struct.pack("<H", len(extra)) + extra)
    gz = hdr + b"".join(c for c, _ in segments) + struct.pack(
        "<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) % (1 << 32))
    assert zlib.decompress(gz, 31) == data
    return gz, data


def flip_bit_refused(comp, expect):
    """`comp` with one bit flipped, the first at or after the middle that
    leaves zlib unable to decode `expect` bytes."""
    for bit in range(4 * len(comp), 8 * len(comp)):
        bad = bytearray(comp)
        bad[bit >> 3] ^= 1 << (bit & 7)
        if zlib_refuses(bytes(bad), expect):
            return bytes(bad)
    raise AssertionError("no refused bit flip")


valid_segments()
malformed_segments()
