"""Shared cases for the differential tests of the LZ4 block decoder (no
tests here, and no GPU code): an independent reference decoder written from
the format description alone, a block builder that plays its sequences
forward, and the case families. tests/test_lz4_cases.py checks every case
on the CPU (reference, pyarrow, the host build of csrc/lz4_core.h);
tests/test_gpu_lz4_kernel.py sends what passed there through the kernel.

A raw case is (name, comp, want): one raw LZ4 block and the bytes it
produces. A container case is (name, block, want): the chunks of one
container block, each a u32 big-endian comp_len and a raw block (the layout
io/paths.py lz4_walk describes, without the block's own raw_len word).
Every family is deterministic from its own seed; literals are random bytes,
so a copy at a wrong period or shift cannot go unnoticed. A family is
built once and the same list handed to every caller: do not modify it."""

import functools
import struct

import numpy as np
import pyarrow as pa

LIB = pa.Codec("lz4_raw")

# cause codes of csrc/lz4_core.h
(LZ_OFFSET_ZERO, LZ_OFFSET_FAR, LZ_LENGTH_PAST_INPUT, LZ_LITERAL_PAST_INPUT,
 LZ_OUTPUT_OVERRUN, LZ_INPUT_SHORT, LZ_INPUT_LEFT, LZ_CHUNK_PAST_BLOCK,
 LZ_BLOCK_SHORT, LZ_BLOCK_INPUT_LEFT) = range(1, 11)

WINDOW = 4096  # lz4_core.h kWindow: the input a wave stages at a time
# engine/gpu.py LZ4_MAX_BLOCK_RAW (the GPU tier asserts they are equal)
LZ4_MAX_BLOCK_RAW = 1 << 20


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------

def ref_decode(comp, cap):
    """The bytes of raw LZ4 block `comp` when they fit `cap`, else None.

    Written from the format: sequences of token, optional literal-length
    bytes, literals, 2-byte little-endian offset, optional match-length
    bytes; the last sequence ends behind its literals, exactly at the end
    of the input. None for a length or offset field or a literal that runs
    past the input, offset 0 or before the block's start, output beyond
    `cap`, or input that does not end with a literals-only sequence."""
    comp = bytes(comp)
    n = len(comp)
    out = bytearray()
    ip = 0

    def length(v, ip):
        if v == 15:
            while True:
                if ip >= n:
                    return None, ip
                b = comp[ip]
                ip += 1
                v += b
                if b != 255:
                    break
        return v, ip

    while True:
        if ip >= n:
            return None
        token = comp[ip]
        ip += 1
        lit, ip = length(token >> 4, ip)
        if lit is None or lit > n - ip or len(out) + lit > cap:
            return None
        out += comp[ip:ip + lit]
        ip += lit
        if ip == n:
            return bytes(out)
        if n - ip < 2:
            return None
        off = comp[ip] | comp[ip + 1] << 8
        ip += 2
        mlen, ip = length(token & 15, ip)
        if mlen is None:
            return None
        mlen += 4
        if off == 0 or off > len(out) or len(out) + mlen > cap:
            return None
        period = bytes(out[len(out) - off:])
        out += (period * (mlen // off + 1))[:mlen]


def ref_container(block, raw_len):
    """The bytes of one container block's chunks, or None: every chunk is
    decoded with what the block still misses as its cap, and the chunks
    must yield exactly raw_len bytes and use exactly len(block)."""
    block = bytes(block)
    out = bytearray()
    ip = 0
    while len(out) < raw_len:
        if len(block) - ip < 4:
            return None
        (clen,) = struct.unpack_from(">I", block, ip)
        ip += 4
        if clen > len(block) - ip:
            return None
        got = ref_decode(block[ip:ip + clen], raw_len - len(out))
        if got is None:
            return None
        out += got
        ip += clen
    return bytes(out) if ip == len(block) else None


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------

def _ext(n):
    """The length bytes behind a nibble of 15."""
    return b"" if n < 15 else b"\xff" * ((n - 15) // 255) + bytes([(n - 15) % 255])


def seq(literals, offset=None, match_len=0):
    """One LZ4 sequence; offset None = a block's last one, literals only."""
    m = 0 if offset is None else match_len - 4
    out = bytes([min(len(literals), 15) << 4 | min(m, 15)]) + _ext(len(literals)) + literals
    return out if offset is None else out + struct.pack("<H", offset) + _ext(m)


class Rand:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def pick(self, lo, hi):
        """An integer in lo..hi inclusive."""
        return int(self.rng.integers(lo, hi + 1))


class Block:
    """Assembles a raw block sequence by sequence and plays it forward byte
    by byte, so the expected bytes come from the definition of a sequence
    alone. `headers` lists the stream positions of tokens, length bytes and
    offsets."""

    def __init__(self, R):
        self.R = R
        self.comp = bytearray()
        self.out = bytearray()
        self.headers = []

    def seq(self, literals, offset=None, match_len=0):
        if isinstance(literals, int):
            literals = self.R(literals)
        s = seq(literals, offset, match_len)
        at = len(self.comp)
        nl = 1 + len(_ext(len(literals)))
        self.headers += range(at, at + nl)
        self.headers += range(at + nl + len(literals), at + len(s))
        self.comp += s
        self.out += literals
        if offset is not None:
            assert 0 < offset <= len(self.out) and match_len >= 4
            out = self.out
            for _ in range(match_len):
                out.append(out[-offset])
        return self

    def upto(self, t):
        """Sequences that end exactly at stream byte t: the next token is
        byte t."""
        while t - len(self.comp) >= 274:
            # at most min(..) bytes: 3, up to 16 length bytes, the literal
            self.seq(min(t - len(self.comp) - 100, 4000) - 19, 5, 4)
        left = t - len(self.comp)
        # token, one length byte, the literal, the offset
        assert 19 <= left < 274, left
        self.seq(left - 4, 5, 4)
        assert len(self.comp) == t
        return self

    def shorts(self, count, max_lit=20):
        """`count` short sequences: literals of 0..max_lit bytes, matches
        of 4..40 bytes at offsets up to 200."""
        R = self.R
        if not self.out:
            self.seq(R.pick(1, max_lit), 1, 4)
        for _ in range(count):
            lit = R.pick(0, max_lit)
            self.seq(lit, R.pick(1, min(len(self.out) + lit, 200)), R.pick(4, 40))
        return self

    def tail(self):
        """The 12-byte literal the format's end-of-block rules ask for."""
        return self.seq(12)

    def case(self, name):
        return (name, bytes(self.comp), bytes(self.out))


def chunks(*comps):
    """The chunk run of a container block around raw blocks."""
    return b"".join(struct.pack(">I", len(c)) + c for c in comps)


def one_chunk(comp):
    return chunks(comp)


# ---------------------------------------------------------------------------
# families of valid blocks
# ---------------------------------------------------------------------------

def period_block(off):
    """What match_copy lays out before it doubles."""
    return (63 // off + 1) * off if off < 64 else off


@functools.lru_cache(None)
def match_sweep():
    """One block per (offset, match length): the prefix literal, the match,
    the tail. Offsets around the off < 64 switch and the powers of two,
    lengths around the period block, twice and four times it; the prefix
    moves the destination over every residue mod 8."""
    R = Rand(101)
    cases = []
    k = 0
    for off in list(range(1, 73)) + [126, 127, 128, 129, 255, 256, 4095, 4096, 4097, 65535]:
        d = period_block(off)
        lens = {4, 5, 7, 8, 9, 15, 16, 17, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1,
                4 * d + 3, 1000}
        for n in sorted(x for x in lens if x >= 4):
            r = k % 8
            k += 1
            cases.append(Block(R).seq(max(off, 8) + r, off, n).tail()
                         .case(f"off{off}_len{n}_r{r}"))
    for off in (1, 7, 8, 9, 63, 64, 65):
        d = period_block(off)
        for n in (d, 2 * d + 1):
            for r in range(8):
                cases.append(Block(R).seq(max(off, 8) + r, off, n).tail()
                             .case(f"off{off}_len{n}_every_r{r}"))
    return cases


@functools.lru_cache(None)
def literal_sweep():
    """The literal under test starts at every residue mod 8 of the window
    (the first sequence's literal length moves it) and, independently, at
    every residue of the output (the first match's length moves that):
    all 64 pairs for every length."""
    R = Rand(102)
    cases = []
    for n in list(range(1, 18)) + [63, 64, 65, 511, 512, 513]:
        pairs = set()
        for a in range(4, 12):
            for j in range(8):
                b = Block(R).seq(a, 3, 4 + j)
                op = len(b.out)
                start = len(b.comp) + 1 + len(_ext(n))  # where the literal lies
                b.seq(n, 9, 5).tail()
                assert bytes(b.comp[start:start + n]) == bytes(b.out[op:op + n])
                pairs.add((start % 8, op % 8))
                cases.append(b.case(f"lit{n}_woff{start % 8}_op{op % 8}"))
        assert pairs == {(w, o) for w in range(8) for o in range(8)}, n
    return cases


LONG_MATCH = 300  # 15 in the nibble and the bytes 255, 26


@functools.lru_cache(None)
def window_edges():
    R = Rand(103)
    cases = []
    # the token at stream byte t, then a literal and a match with length
    # bytes: the window's edge falls in each part of the sequence in turn
    for t in range(WINDOW - 8, WINDOW + 5):
        for lit in (0, 1, 3, 9, 15, 273):
            cases.append(Block(R).upto(t).seq(lit, 30, LONG_MATCH).shorts(3).tail()
                         .case(f"token_at_{t}_lit{lit}"))
    # a literal that ends one byte inside the window, on its last byte
    # (the one read of the window's slack words) and one byte past it (the
    # input -> output path)
    for end in (WINDOW - 1, WINDOW, WINDOW + 1):
        b = Block(R).seq(10, 3, 4)
        n = end - len(b.comp) - 17  # token and 16 length bytes
        assert len(_ext(n)) == 16
        b.seq(n, 77, 10)
        assert len(b.comp) - 2 == end
        cases.append(b.shorts(6).tail().case(f"literal_ends_at_{end}"))
    # a literal longer than the window goes input -> output and the window
    # restarts behind it, at every residue of the input pointer
    for k in range(9):
        cases.append(Block(R).seq(5, 2, 4).seq(WINDOW + k, 100, 20).shorts(12).tail()
                     .case(f"bypass_{WINDOW + k}"))
    b = Block(R)
    while len(b.comp) < 3 * WINDOW + 700:
        b.shorts(50)
    cases.append(b.tail().case("three_refills"))
    n = 15 + 299 * 255 + 40  # 300 length bytes
    assert len(_ext(n)) == 300
    b = Block(R).upto(WINDOW - 150).seq(n, 65535, LONG_MATCH)
    cases.append(b.shorts(5).tail().case("length_bytes_300_over_refill"))
    return cases


@functools.lru_cache(None)
def chunked():
    """Container blocks: (name, chunk run, bytes)."""
    R = Rand(104)

    def blk(lit, off, n):
        b = Block(R).seq(lit, off, n).tail()
        if len(b.comp) % 2 == 0:  # odd bodies: what follows sits odd
            b = Block(R).seq(lit + 1, off, n).tail()
        assert len(b.comp) % 2 == 1
        return bytes(b.comp), bytes(b.out)

    a, b, c, d, e = blk(33, 7, 90), blk(70, 64, 200), blk(9, 1, 1000), blk(200, 129, 60), blk(15, 3, 4)
    big = Block(R).seq(3000, 5, 300).seq(1500, 70, 400).shorts(40).tail()
    assert len(big.comp) >= WINDOW + 1
    big = (bytes(big.comp), bytes(big.out))
    # after `big` the window holds the end of ITS input; the small chunk
    # must be read from its own bytes
    small = Block(R).seq(6, 2, 9).seq(3, 4, 5).tail()
    small = (bytes(small.comp), bytes(small.out))
    empty = (b"\x00", b"")  # a lone token: no literals, the block's end

    def case(name, *parts):
        return (name, chunks(*(p[0] for p in parts)), b"".join(p[1] for p in parts))

    return [case("one_chunk", a), case("two_chunks", a, b),
            case("five_chunks", a, b, c, d, e),
            case("empty_chunk_in_the_middle", a, empty, b),
            case("big_then_small", big, small),
            case("small_big_small", small, big, small)]


TEXT = b"".join(b"row-%d,name=%d;" % (i, i % 7) for i in range(4000))


def example_image(rows=200):
    from bench import make_batch
    from spark_tfrecord_amd.engine import cpu as cpu_engine

    return bytes(cpu_engine.encode_batch(make_batch(rows, seed=3), "Example"))


@functools.lru_cache(None)
def encoder_streams():
    """What the library's encoder makes of inputs that steer it to long
    runs, short and long periods, one bypassed literal, and a block of the
    largest size the device takes."""
    R = Rand(105)
    n = 64 << 10
    mixed = bytearray()
    while len(mixed) < LZ4_MAX_BLOCK_RAW:
        at = (len(mixed) * 7) % (len(TEXT) - 4096)
        mixed += TEXT[at:at + 4096] + R(1024)
    datas = [("zeros", bytes(n)),
             ("period_3", (R(3) * n)[:n]),
             ("period_64", (R(64) * n)[:n]),
             ("period_65", (R(65) * n)[:n]),
             ("random", R(n)),
             ("text", TEXT),
             ("example_200_rows", example_image(200)),
             ("max_block_raw", bytes(mixed[:LZ4_MAX_BLOCK_RAW]))]
    return [(name, LIB.compress(d, asbytes=True), d) for name, d in datas]


# ---------------------------------------------------------------------------
# malformed blocks
# ---------------------------------------------------------------------------

def _long_prefix(R):
    """More than a window of valid sequences with doubling rounds in them."""
    b = Block(R).seq(3000, 5, 300).seq(1500, 70, 400)
    assert len(b.comp) > WINDOW + 400
    return b


@functools.lru_cache(None)
def malformed():
    """Raw blocks the core refuses: (name, comp, cap, cause), the cause
    stated by hand. The seven causes lie behind a window refill and behind
    doubling rounds, where the short blocks of test_lz4_codec.py never
    get."""
    R = Rand(106)
    L = b"lz4-block-hdr"
    pre = _long_prefix(R)
    head, P = bytes(pre.comp), len(pre.out)
    tail = seq(b"the-last-12b")
    N = P + 13 + 20 + 12
    out = [
        ("offset_zero", head + seq(L, 0, 20) + tail, N, LZ_OFFSET_ZERO),
        ("offset_before_block", head + seq(L, P + 14, 20) + tail, N, LZ_OFFSET_FAR),
        ("length_bytes_cut", head + b"\xf0\xff\xff", N, LZ_LENGTH_PAST_INPUT),
        ("match_length_bytes_cut", head + seq(L, 7, 19 + 255)[:-1], N + 300,
         LZ_LENGTH_PAST_INPUT),
        ("literal_cut", head + seq(L)[:-1], N, LZ_LITERAL_PAST_INPUT),
        ("output_overrun", head + seq(L, 7, 30) + tail, N, LZ_OUTPUT_OVERRUN),
        ("match_overrun", head + seq(L, 7, 21) + tail, P + 13 + 20, LZ_OUTPUT_OVERRUN),
        ("no_last_sequence", head + seq(L, 7, 20), N, LZ_INPUT_SHORT),
        ("offset_cut", head + seq(L, 7, 8)[:-1], N, LZ_INPUT_SHORT),
        ("input_left", head + seq(L, 7, 20) + tail + b"\x00\x00\x00", N, LZ_INPUT_LEFT),
        ("match_70000_into_45", seq(L, 7, 70000) + tail, 13 + 20 + 12, LZ_OUTPUT_OVERRUN),
        ("literal_5000_into_45", seq(R(5000)), 45, LZ_OUTPUT_OVERRUN),
        ("empty_input", b"", 45, LZ_INPUT_SHORT),
    ]
    assert {c[3] for c in out} == set(range(1, 8))
    return out


@functools.lru_cache(None)
def malformed_containers():
    """Container blocks the chunk walk refuses: (name, chunk run, raw_len,
    cause)."""
    R = Rand(107)
    a = Block(R).seq(5000, 100, 600).tail()
    b = Block(R).seq(9, 2, 40).tail()
    ac, bc = bytes(a.comp), bytes(b.comp)
    na, nb = len(a.out), len(b.out)
    three = chunks(ac, bc, ac)
    # blocks are independent: the second chunk's first match may not reach
    # into what the first chunk produced
    reach = seq(R(5), 6, 8) + seq(R(12))
    return [
        ("comp_len_past_block", b"\x7f" + three[1:], 2 * na + nb, LZ_CHUNK_PAST_BLOCK),
        ("last_comp_len_one_more", chunks(ac, bc) + struct.pack(">I", len(ac) + 1) + ac,
         2 * na + nb, LZ_CHUNK_PAST_BLOCK),
        ("chunk_header_cut", chunks(ac, bc) + b"\x00\x00\x00", 2 * na + nb,
         LZ_CHUNK_PAST_BLOCK),
        ("block_short", three, 2 * na + nb + 1, LZ_BLOCK_SHORT),
        ("block_input_left", three, na + nb, LZ_BLOCK_INPUT_LEFT),
        ("second_chunk_overruns", three, na + nb - 1, LZ_OUTPUT_OVERRUN),
        ("match_into_previous_chunk", chunks(ac, reach), na + 5 + 8 + 12, LZ_OFFSET_FAR),
        ("match_into_previous_big_chunk", chunks(bytes(_long_prefix(R).tail().comp), reach),
         3000 + 300 + 1500 + 400 + 12 + 5 + 8 + 12, LZ_OFFSET_FAR),
    ]


# ---------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------

MUTANT_SEED = 108


def random_block(R, comp_len):
    """A valid block of about comp_len bytes: mixed literal lengths, offsets
    and match lengths."""
    b = Block(R)
    lit = R.pick(1, 30)
    while len(b.comp) < comp_len:
        op = len(b.out) + lit
        kind = R.pick(0, 9)
        off = (R.pick(1, min(op, 8)) if kind < 3 else R.pick(1, min(op, 70)) if kind < 6
               else R.pick(1, min(op, 65535)))
        kind = R.pick(0, 19)
        n = R.pick(4, 18) if kind < 12 else R.pick(19, 300) if kind < 19 else 1000
        b.seq(lit, off, n)
        kind = R.pick(0, 19)
        lit = (0 if kind < 3 else R.pick(1, 14) if kind < 13 else R.pick(15, 40) if kind < 18
               else 300 if kind < 19 else 1000)
    return b.tail()


@functools.lru_cache(None)
def mutants():
    """Single-byte mutations of eight valid blocks: (name, comp, cap, want)
    with cap the unmutated block's length and want = ref_decode(comp, cap),
    None for a block that must be refused. Half of a block's 32 mutations
    land on header bytes (tokens, length bytes, offsets), half anywhere.
    The first entry of every block is the block itself."""
    R = Rand(MUTANT_SEED)
    out = []
    for k in range(8):
        b = random_block(R, 5000 + 600 * k)
        assert 5000 <= len(b.comp) <= 10240
        comp, cap = bytes(b.comp), len(b.out)
        out.append((f"block{k}", comp, cap, bytes(b.out)))
        for m in range(32):
            at = b.headers[R.pick(0, len(b.headers) - 1)] if m % 2 == 0 else R.pick(0, len(comp) - 1)
            mut = bytearray(comp)
            mut[at] ^= R.pick(1, 255)
            mut = bytes(mut)
            out.append((f"block{k}_byte{at}_{mut[at]:02x}", mut, cap, ref_decode(mut, cap)))
    return out
