"""Shared cases for the frame-discovery tests (no tests here): a plain
reference of the candidate scan and of the chain check, and small file
images that put frame heads, fake heads and the file's end where the scan
kernel's index math changes.

The reference tests every byte position on its own, with a table CRC32C
kept in this module: it shares nothing with the kernel (16 positions per
lane out of four aligned words, a byte-wise tail, per-range chunk rounding,
a block-local slot scan) and nothing with the project's CRC code.

One block of the scan covers 256 lanes x 16 positions = 4096 bytes, so
every image is a few blocks long."""

import struct
from typing import NamedTuple, Tuple

import numpy as np

BLOCK_BYTES = 4096  # positions one block of the scan kernel covers
CHUNK = 16          # positions one lane covers


# ---------------------------------------------------------------------------
# CRC32C (Castagnoli, reflected polynomial 0x82F63B78), one table, bytewise
# ---------------------------------------------------------------------------

def _make_table():
    tab = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        tab.append(c)
    return tab


_TAB = _make_table()


def crc32c(data: bytes) -> int:
    c = 0xFFFFFFFF
    for b in data:
        c = _TAB[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc(data: bytes) -> int:
    """TFRecord's masked CRC32C: rotate right by 15, add a constant."""
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def header(length: int) -> bytes:
    """The 12 bytes that make a position a candidate: u64 length + its
    masked CRC. Also what a decoy is made of."""
    h = struct.pack("<Q", length)
    return h + struct.pack("<I", masked_crc(h))


def frame(payload: bytes) -> bytes:
    return header(len(payload)) + payload + struct.pack("<I", masked_crc(payload))


def filler(n: int, seed: int) -> bytes:
    """n payload bytes, all >= 0x80: every u64 read out of them is far
    beyond any image here, so filler never yields a candidate of its own."""
    return np.random.default_rng(seed).integers(0x80, 0x100, n).astype(
        np.uint8).tobytes()


# ---------------------------------------------------------------------------
# Reference
# ---------------------------------------------------------------------------

def ref_candidates(img: bytes, ranges):
    """(pos, len) int64 arrays of every position i inside a range with
    i + 16 <= N whose u64 length is <= N - i - 16 and whose next u32 is the
    masked CRC32C of those 8 bytes; range by range, ascending inside each."""
    N = len(img)
    a = np.frombuffer(img, np.uint8)
    if N < 16:
        z = np.zeros(0, np.int64)
        return z, z.copy()
    M = N - 15  # positions 0 .. N - 16
    win = np.lib.stride_tricks.sliding_window_view(a, 12)[:M]
    lens = np.ascontiguousarray(win[:, :8]).view("<u8").ravel()
    want = np.ascontiguousarray(win[:, 8:]).view("<u4").ravel()
    room = np.uint64(N - 16) - np.arange(M, dtype=np.uint64)
    fits = np.nonzero(lens <= room)[0]
    good = np.array([i for i in fits
                     if masked_crc(img[i:i + 8]) == int(want[i])], np.int64)
    pos = []
    for s, e in ranges:
        pos.append(good[(good >= s) & (good < e)])
    pos = np.concatenate(pos) if pos else np.zeros(0, np.int64)
    return pos, lens[pos].astype(np.int64)


def ref_chain(pos, lens, carry_in: int):
    """What the chain check makes of candidates (pos, lens) that follow a
    chain ending at carry_in: (off, carry_out, broken). carry_out is None
    for no candidates: the word is then left alone."""
    pos = np.asarray(pos, np.int64)
    lens = np.asarray(lens, np.int64)
    if pos.size == 0:
        return pos.copy(), None, False
    ends = pos + 16 + lens
    want = np.concatenate([[carry_in], ends[:-1]])
    return pos + 12, int(ends[-1]), bool((pos != want).any())


def walk(img: bytes):
    """Frame heads by following the lengths from 0 (no CRC test):
    (pos, len) of the frames of a well-formed image."""
    pos, lens = [], []
    cur = 0
    while cur < len(img):
        (n,) = struct.unpack_from("<Q", img, cur)
        pos.append(cur)
        lens.append(n)
        cur += 16 + n
    assert cur == len(img)
    return np.array(pos, np.int64), np.array(lens, np.int64)


# ---------------------------------------------------------------------------
# Images
# ---------------------------------------------------------------------------

class Case(NamedTuple):
    img: bytes
    # planted fake headers that pass the scan, (pos, len) ascending
    decoys: Tuple[Tuple[int, int], ...] = ()
    # the well-formed frames end here; the rest is trailing garbage
    valid: int = -1

    @property
    def torn(self) -> bool:
        return self.valid != len(self.img)

    def frames(self):
        return walk(self.img[:self.valid])

    def expected(self):
        """Frames plus decoys, ascending: what a scan of (0, N) must give."""
        pos, lens = self.frames()
        if self.decoys:
            d = np.array(self.decoys, np.int64)
            pos = np.concatenate([pos, d[:, 0]])
            lens = np.concatenate([lens, d[:, 1]])
            order = np.argsort(pos, kind="stable")
            pos, lens = pos[order], lens[order]
        return pos, lens


def _case(img: bytes, decoys=(), garbage: int = 0) -> Case:
    valid = len(img)
    if garbage:
        img += filler(garbage, 900 + garbage)
    return Case(img, tuple(sorted(decoys)), valid)


def frames_of(payload_lens, seed=1) -> bytes:
    return b"".join(frame(filler(n, seed + k))
                    for k, n in enumerate(payload_lens))


def image_with_heads(heads, N: int, plants=(), seed=1) -> bytes:
    """Frames whose heads sit at `heads` (ascending from 0) in an image of N
    bytes. `plants` = [(position, length word)]: a fake 12-byte header is
    laid over the filler there; it must lie inside one payload."""
    heads = list(heads)
    assert heads[0] == 0 and heads == sorted(heads)
    out = bytearray()
    for k, h in enumerate(heads):
        end = heads[k + 1] if k + 1 < len(heads) else N
        n = end - h - 16
        assert n >= 0, (h, end)
        payload = bytearray(filler(n, seed + k))
        for p, length in plants:
            if h <= p < end:
                o = p - (h + 12)
                assert 0 <= o and o + 12 <= n, (p, h, end)
                payload[o:o + 12] = header(length)
        out += frame(bytes(payload))
    assert len(out) == N
    return bytes(out)


def split_sizes(N: int):
    """Payload lengths of frames that fill exactly N >= 16 bytes: short
    frames of varying size, the last one takes what is left."""
    out = []
    k = 0
    while N >= 16 + 16 + 22:
        n = (7 * k) % 23
        out.append(n)
        N -= 16 + n
        k += 1
    out.append(N - 16)
    return out


TAIL_SIZES = (16, 17, 31, 32, 33, 47, 48, 4095, 4096, 4097, 4111, 4112)


def _tail_cases():
    out = {}
    for N in TAIL_SIZES:
        out[f"tail_{N}"] = _case(frames_of(split_sizes(N), seed=N))
        if N > 16:
            # the same size, its last 1..15 bytes garbage
            g = min(N - 16, 1 + (N * 5) % 15)
            out[f"tail_{N}_torn{g}"] = _case(
                frames_of(split_sizes(N - g), seed=N), garbage=g)
    return out


def _phase_case():
    # 17-byte frames walk the head through every phase of a chunk, 21-byte
    # frames do it in another order
    img = frames_of([1] * 40 + [5] * 40, seed=50)
    pos, _ = walk(img)
    assert set(pos[:40] % CHUNK) == set(range(16))
    assert set(pos[40:] % CHUNK) == set(range(16))
    return _case(img)


def _boundary_cases():
    B = BLOCK_BYTES
    return {
        # 4088: length word ends block 0, its CRC opens block 1; 2B - 1: the
        # last position of block 1; 3B: the first position of block 3
        "boundary_straddle": _case(image_with_heads(
            [0, B - 8, 2 * B - 1, 3 * B], 3 * B + 16 + 7, seed=60)),
        # B - 1 and 2B: last of block 0, first of block 2; 3B - 12: the
        # header ends with the block
        "boundary_edges": _case(image_with_heads(
            [0, B - 1, 2 * B, 3 * B - 12], 3 * B + 40, seed=70)),
        "boundary_first_of_block": _case(image_with_heads(
            [0, B, B + 16], B + 32, seed=80)),
    }


def _zero_length_cases():
    z = frame(b"")
    assert len(z) == 16
    return {
        "zero_alone": _case(z),
        # a candidate in every lane of block 0 and in 44 lanes of block 1
        "zero_x300": _case(z * 300),
        # every lane of two whole blocks, and 8 lanes of a third
        "zero_x520": _case(z * 520),
        "zero_last": _case(frames_of([33, 7], seed=90) + z),
    }


def _decoy_cases():
    B = BLOCK_BYTES
    out = {}
    # A payload that is a run of fake headers, 12 bytes apart: positions p
    # and p + 12 share a chunk whenever p % 16 <= 3, so lanes with two
    # candidates alternate with lanes with one. (Three in one chunk would
    # need overlapping headers, i.e. a CRC that is itself a small length.)
    lens = [5, 0, 3, 40, 1, 0, 9, 2] * 5
    run = b"".join(header(n) for n in lens)
    img = (frames_of([3], seed=100) + frame(run)
           + frames_of([60, 0, 11], seed=101))
    start = 16 + 3 + 12
    decoys = [(start + 12 * k, n) for k, n in enumerate(lens)]
    assert sum(1 for p, _ in decoys if p % 16 <= 3) >= 8
    out["decoy_run"] = _case(img, decoys)

    # fake headers on either side of a block boundary, and one across it
    plants = [(B - 24, 7), (B - 12, 0), (B, 2), (2 * B - 5, 1)]
    out["decoy_boundary"] = _case(
        image_with_heads([0, B - 100, 2 * B - 50, 2 * B + 300],
                         2 * B + 400, plants, seed=110), plants)

    # a fake header whose length leads exactly to the next real head: its
    # own link holds, only the walk from 0 leaves it out
    heads = [0, 500, 900]
    d = 100
    plants = [(d, heads[1] - d - 16)]
    out["decoy_points_at_head"] = _case(
        image_with_heads(heads, 1000, plants, seed=120), plants)
    return out


def _cull_case():
    # Fake headers with a valid CRC whose length word sits on the cull's
    # edge: N - i - 16 is kept (the frame would end with the file),
    # N - i - 15 is culled, as are lengths with bit 63 set, which must not
    # wrap into range.
    N = 3 * BLOCK_BYTES + 123
    heads = [0, 700, BLOCK_BYTES + 3, 2 * BLOCK_BYTES + 77]
    at = [40, 333, 800, BLOCK_BYTES + 40, BLOCK_BYTES + 1001,
          2 * BLOCK_BYTES + 100, N - 16]
    plants = [
        (at[0], N - at[0] - 16),      # kept
        (at[1], N - at[1] - 15),      # culled: one byte too long
        (at[2], 2 ** 63),             # culled
        (at[3], 2 ** 64 - 1),         # culled
        (at[4], N - at[4] - 16),      # kept
        (at[5], 2 ** 63 + 5),         # culled
        (at[6], N - at[6] - 16),      # kept, near the end: length 0
    ]
    img = image_with_heads(heads, N, plants, seed=130)
    kept = [(p, n) for p, n in plants if n == N - p - 16]
    assert kept[-1][1] == 0 and len(kept) == 3
    return _case(img, kept)


def _garbage_cases():
    return {f"garbage_{n}": filler(n, 140 + n) for n in (1, 15, 16, 100, 5000)}


def _big_case():
    # ~70 KiB: 17 blocks, frames of many sizes, a few of them empty
    rng = np.random.default_rng(150)
    sizes = [int(x) for x in rng.integers(0, 400, 330)]
    sizes[10] = sizes[200] = 0
    return _case(frames_of(sizes, seed=151))


def _build_cases():
    out = {"phase": _phase_case(), "cull": _cull_case(), "big": _big_case()}
    out.update(_boundary_cases())
    out.update(_zero_length_cases())
    out.update(_tail_cases())
    out.update(_decoy_cases())
    return out


CASES = _build_cases()
GARBAGE = _garbage_cases()
# the cases whose file end takes the byte-wise branch worth pinning against
# the word branch (every image's last chunks take it; these vary the end)
TAIL_CASES = [k for k in CASES if k.startswith("tail_")]
PAD = 32  # zero bytes that turn a file's tail chunks into interior ones


def range_sets(name: str):
    """Range lists to scan CASES[name] with, each ascending and disjoint
    (they need not cover the image). All land in one candidate array."""
    case = CASES[name]
    N = len(case.img)
    sets = {"whole": [(0, N)]}
    if N < 128:
        cuts = sorted({0, 1, N - 16, N})
        if len(cuts) > 2:
            sets["split_odd"] = list(zip(cuts[:-1], cuts[1:]))
        return sets
    # splits that are no multiple of 16
    if N > 8200:
        sets["split_odd"] = [(0, 4099), (4099, 8200), (8200, N)]
    else:
        a, b = (N // 3) | 1, (2 * N // 3) | 1
        sets["split_odd"] = [(0, a), (a, b), (b, N)]
    pos, _ = case.expected()
    h = int(pos[len(pos) // 2])
    # a split inside a frame header: the head belongs to the range that
    # holds its first byte
    sets["split_in_header"] = [(0, h + 5), (h + 5, N)]
    # one-byte ranges: on a head, and on the byte after it
    sets["one_byte"] = [(h, h + 1), (h + 1, h + 2)]
    # ranges that start late, leave a gap and end before N
    sets["gaps"] = [(19, N // 2), (N // 2 + 33, N - 20)]
    return sets


def chain_cases(C: int, carry_in: int):
    """Synthetic candidate arrays of C entries chained on from carry_in:
    {name: (pos, lens)}. Every broken one has a single mismatch."""
    rng = np.random.default_rng(C)
    lens = rng.integers(1, 90, C).astype(np.int64)
    ends = carry_in + np.cumsum(16 + lens)
    pos = np.concatenate([[carry_in], ends[:-1]]).astype(np.int64)
    out = {"clean": (pos, lens)}

    def bump(k):
        # candidate k starts one byte late and is one byte shorter: link k
        # is the only one that breaks, the link after it still holds
        p, n = pos.copy(), lens.copy()
        p[k] += 1
        n[k] -= 1
        return p, n

    out["first"] = bump(0)
    out["last"] = bump(C - 1)
    if C > 256:
        out["block_edge"] = bump(256)  # first candidate of the second block
        out["block_edge_prev"] = bump(255)
    return out
