"""Differential GPU tests of unlz4_blocks_kernel (csrc/hip/lz4.hip): the
families of tests/lz4_cases.py through `_native.gpu_unlz4_blocks` with block
tables built here, so the test chooses every block's place in the input and
the output (all 64 pairs of `in_off & 7` and `out_off & 7`), its file and
the launch's `max_waves`. Every comparison is exact bytes (against the bytes
the case states, and against the host build of the same core) or an exact
error word. Outputs stand between guard bytes that must survive every
launch, refused blocks included. tests/test_lz4_cases.py checks the same
cases on the CPU; this module checks again, with the plain-Python reference
and the host core, every block it sends."""

import functools
import struct

import numpy as np
import pytest

import lz4_cases as C
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
GUARD = 16
GUARD_BYTE = 0xEE


def _gpu_engine():
    from spark_tfrecord_amd.engine import gpu
    return gpu


class Launch:
    """One launch over blocks = [(chunk run, raw_len, file)]; a file's
    blocks are consecutive. Block i has in_off & 7 == i mod 8 and
    out_off & 7 == (i div 8) mod 8; at least GUARD bytes of GUARD_BYTE lie
    before, between and behind the outputs."""

    def __init__(self, blocks):
        import torch

        self.blocks = blocks
        n = len(blocks)
        assert int(_native.LZ4_BLOCK_COLS) == 5
        self.table = np.zeros((n, 5), np.int64)
        ipos, opos = 0, GUARD
        for i, (run, raw_len, fi) in enumerate(blocks):
            ipos = -(-ipos // 8) * 8 + i % 8
            opos = -(-opos // 8) * 8 + (i // 8) % 8
            self.table[i] = (ipos, len(run), opos, raw_len, fi)
            ipos += len(run)
            opos += raw_len + GUARD
        comp = np.zeros(ipos + 8, np.uint8)
        self.guard = np.ones(opos, bool)
        for (run, raw_len, _), row in zip(blocks, self.table):
            comp[row[0]:row[0] + len(run)] = np.frombuffer(run, np.uint8)
            self.guard[row[2]:row[2] + raw_len] = False
        files = self.table[:, 4]
        self.nfile = int(files.max()) + 1 if n else 1
        assert n == 0 or (files[0] == 0 and set(np.diff(files)) <= {0, 1})
        self.block0 = np.searchsorted(files, np.arange(self.nfile)).astype(np.int64)
        self.comp = torch.as_tensor(comp).to(DEVICE)
        self.out = torch.full((opos,), GUARD_BYTE, dtype=torch.uint8, device=DEVICE)
        self.err = torch.full((self.nfile,), -1, dtype=torch.int64, device=DEVICE)
        self.table_d = torch.as_tensor(self.table).to(DEVICE)
        self.block0_d = torch.as_tensor(self.block0).to(DEVICE)
        # the launcher trusts the table: every extent inside its buffer,
        # the outputs disjoint with their guards between them
        t = self.table
        if n:
            assert t.min() >= 0 and t[:, 4].max() < self.err.numel()
            assert (t[:, 0] + t[:, 1]).max() <= self.comp.numel()
            assert (t[:, 2] + t[:, 3]).max() + GUARD <= self.out.numel()
            assert t[0, 2] >= GUARD
            assert (t[1:, 2] - (t[:-1, 2] + t[:-1, 3]) >= GUARD).all()
            assert (self.block0 >= 0).all() and (self.block0 < n).all()
        assert int(self.guard.sum()) >= GUARD * (n + 1)

    def residues(self):
        return {(int(r[0]) & 7, int(r[2]) & 7) for r in self.table}

    def run(self, max_waves=None, nblock=None):
        """([each block's bytes], [each file's error word])"""
        import torch

        g = _gpu_engine()
        _native.gpu_unlz4_blocks(
            self.comp.data_ptr(), self.table_d.data_ptr(), self.block0_d.data_ptr(),
            len(self.blocks) if nblock is None else nblock, self.out.data_ptr(),
            self.err.data_ptr(),
            g._lz4_max_waves(DEVICE) if max_waves is None else max_waves,
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self.collect()

    def collect(self):
        flat = self.out.cpu().numpy()
        spoiled = np.flatnonzero(flat[self.guard] != GUARD_BYTE)
        assert spoiled.size == 0, f"{spoiled.size} guard bytes overwritten"
        return ([flat[r[2]:r[2] + r[3]].tobytes() for r in self.table],
                [int(e) for e in self.err.cpu().numpy()])


# ---------------------------------------------------------------------------
# what is sent, each block checked on the CPU first
# ---------------------------------------------------------------------------

def host_block(comp, cap):
    """(bytes, 0) or (None, cause) of the host core, through the window."""
    try:
        return _native.host_unlz4_block(comp, cap, True), 0
    except RuntimeError as e:
        return None, int(str(e).rsplit(" ", 1)[1])


def clean_raw(cases):
    """[(name, chunk run, want)] of raw cases, as one-chunk blocks."""
    out = []
    for name, comp, want in cases:
        assert C.ref_decode(comp, len(want)) == want, name
        assert host_block(comp, len(want)) == (want, 0), name
        out.append((name, C.one_chunk(comp), want))
    return out


def clean_chunked(cases):
    for name, run, want in cases:
        assert C.ref_container(run, len(want)) == want, name
        assert P.lz4_decompress(struct.pack(">I", len(want)) + run, name) == want, name
    return list(cases)


def refused_raw(cases):
    """[(name, chunk run, raw_len, cause)] of malformed raw blocks."""
    out = []
    for name, comp, cap, cause in cases:
        assert C.ref_decode(comp, cap) is None, name
        assert host_block(comp, cap) == (None, cause), name
        out.append((name, C.one_chunk(comp), cap, cause))
    return out


def refused_chunked(cases):
    for name, run, raw_len, cause in cases:
        assert C.ref_container(run, raw_len) is None, name
        with pytest.raises(ValueError, match="lz4"):
            P.lz4_decompress(struct.pack(">I", raw_len) + run, name)
    return list(cases)


@functools.lru_cache(None)
def family(name):
    if name == "chunked":
        return clean_chunked(C.chunked())
    return clean_raw(getattr(C, name)())


@functools.lru_cache(None)
def spares():
    """Clean blocks to stand between refused ones."""
    return clean_raw(C.literal_sweep()[5::187] + C.window_edges()[::17]) + family("chunked")[2:4]


def decode_each_as_a_file(named, max_waves=None):
    """named = [(name, run, raw_len)] -> the launch's ([bytes], [error word])
    with one file per block."""
    launch = Launch([(run, raw_len, i) for i, (_, run, raw_len) in enumerate(named)])
    return launch, launch.run(max_waves)


# ---------------------------------------------------------------------------
# valid blocks: one launch per family
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["match_sweep", "literal_sweep", "window_edges", "chunked",
                                  "encoder_streams"])
def test_family(name):
    cases = family(name)
    # a small family is sent several times over, for the 64 placements
    cases = cases * -(-64 // len(cases))
    launch, (got, err) = decode_each_as_a_file([(n, run, len(w)) for n, run, w in cases])
    assert len(launch.residues()) == 64
    bad = [n for (n, _, want), have in zip(cases, got) if have != want]
    assert not bad, (len(bad), bad[:10])
    wrong = [(n, e) for (n, _, _), e in zip(cases, err) if e != -1]
    assert not wrong, wrong[:10]


def test_max_block_raw_is_the_encoder_streams_case(tmp_path):
    """The gate, no launch: a block of exactly LZ4_MAX_BLOCK_RAW is for the
    device (test_family[encoder_streams] decodes it), one byte more sends
    the file to the host."""
    g = _gpu_engine()
    assert g.LZ4_MAX_BLOCK_RAW == C.LZ4_MAX_BLOCK_RAW
    name, comp, raw = C.encoder_streams()[-1]
    assert name == "max_block_raw" and len(raw) == g.LZ4_MAX_BLOCK_RAW
    p = tmp_path / "at.tfrecord.lz4"
    p.write_bytes(P.lz4_pack_block(raw))
    meta = g.lz4_device_meta(str(p))
    assert meta is not None and meta[1] == len(raw)
    assert meta[0].tolist() == [[4, len(C.one_chunk(comp)), 0, len(raw)]]
    assert p.read_bytes()[4:] == C.one_chunk(comp)
    over = raw + b"!"
    q = tmp_path / "over.tfrecord.lz4"
    q.write_bytes(P.lz4_pack_block(over))
    assert g.lz4_device_meta(str(q)) is None
    assert P.decompress_file(str(q)) == over


# ---------------------------------------------------------------------------
# refused blocks
# ---------------------------------------------------------------------------

def with_spares(named):
    """A clean block in front of every pair of `named`: (name, run, raw_len,
    word, want), so every third block of the result is a spare."""
    spare = spares()
    out = []
    for k, item in enumerate(named):
        if k % 2 == 0:
            n, run, want = spare[(k // 2) % len(spare)]
            out.append((f"spare_{n}", run, len(want), -1, want))
        out.append(item)
    return out


def check_each(named):
    launch, (got, err) = decode_each_as_a_file([x[:3] for x in named])
    assert len(launch.residues()) == min(64, len(named))
    for (name, _, _, word, want), have, e in zip(named, got, err):
        assert e == word, (name, e, word)
        if want is not None:
            assert have == want, name
    return launch


def test_malformed():
    named = [(n, run, raw_len, (1 << 8) | cause, None) for n, run, raw_len, cause in
             refused_raw(C.malformed()) + refused_chunked(C.malformed_containers())]
    assert {w & 255 for _, _, _, w, _ in named} == set(range(1, 11))
    check_each(with_spares(named))


def test_mutants():
    named = []
    for name, comp, cap, want in C.mutants():
        got, cause = host_block(comp, cap)
        assert got == want, name
        if want is None:
            named.append((name, C.one_chunk(comp), cap, (1 << 8) | cause, None))
        else:
            named.append((name, C.one_chunk(comp), len(want), -1, want))
    words = [w for _, _, _, w, _ in named]
    assert words.count(-1) > 8 and len(words) - words.count(-1) >= 64
    check_each(with_spares(named))


def test_error_word_is_the_first_refused_block_of_its_file():
    spare = spares()
    bad = {c[0]: c for c in refused_raw(C.malformed())}
    # block 1 is refused at its first sequence, block 3 only behind three
    # windows of short sequences and with the lower cause: a word that
    # keeps the last writer, or the lower cause, is not the word of block 1
    _, comp, want = next(c for c in C.window_edges() if c[0] == "three_refills")
    assert comp[-13] == 0xC0  # the tail: a token and 12 literals
    slow = comp[:-13] + C.seq(b"lz4-block-hdr", 0, 20) + C.seq(b"the-last-12b")
    (later,) = refused_raw([("offset_zero_behind_three_refills", slow, len(want) + 33,
                             C.LZ_OFFSET_ZERO)])
    first, last = bad["literal_5000_into_45"], bad["literal_cut"]
    assert len(later[1]) > 3 * C.WINDOW and later[3] < first[3]
    ok = [(run, len(want)) for _, run, want in spare]
    blocks = [ok[0] + (0,), first[1:3] + (0,), ok[1] + (0,), later[1:3] + (0,),  # file A
              ok[2] + (1,), ok[3] + (1,),                                       # file B
              ok[4] + (2,), ok[5] + (2,), last[1:3] + (2,),                     # file C
              ok[6] + (3,)]
    launch = Launch(blocks)
    assert launch.block0.tolist() == [0, 4, 6, 9]
    got, err = launch.run()
    # atomicMin keeps the lower block, whatever its cause
    assert err == [(2 << 8) | first[3], -1, (3 << 8) | last[3], -1]
    for k, s in zip((0, 2, 4, 5, 6, 7, 9), range(7)):
        assert got[k] == spare[s][2], k


# ---------------------------------------------------------------------------
# the launch: grid stride, max_waves, nblock
# ---------------------------------------------------------------------------

@functools.lru_cache(None)
def mixed_blocks():
    """About 40 blocks of mixed sizes, two refused ones among them:
    (name, run, raw_len, word, want)."""
    clean = (family("match_sweep")[7::60] + family("window_edges")[3::20]
             + family("chunked") + clean_raw(C.encoder_streams()[4:7]))
    named = [(n, run, len(w), -1, w) for n, run, w in clean]
    for at, (n, run, raw_len, cause) in zip((5, 30), refused_raw(C.malformed()[1:6:4])):
        named.insert(at, (n, run, raw_len, (1 << 8) | cause, None))
    assert 36 <= len(named) <= 48
    return named


@pytest.fixture(scope="module")
def uncapped():
    named = mixed_blocks()
    return named, check_each(named).collect()


@pytest.mark.parametrize("max_waves", [4, 8])
def test_grid_stride(uncapped, max_waves):
    """One or two workgroups walk all the blocks: the same bytes and words
    as the launch that gives every block its own wave."""
    named, (want_bytes, want_err) = uncapped
    _, (got, err) = decode_each_as_a_file([x[:3] for x in named], max_waves)
    assert err == want_err
    for x, have, want in zip(named, got, want_bytes):
        if x[3] == -1:
            assert have == want == x[4], x[0]


def test_max_waves_below_a_workgroup_launches_nothing():
    named = mixed_blocks()[:8]
    launch = Launch([(run, raw_len, i) for i, (_, run, raw_len, _, _) in enumerate(named)])
    with pytest.raises(ValueError, match="max_waves"):
        launch.run(max_waves=3)
    got, err = launch.collect()
    assert err == [-1] * 8
    assert all(set(b) == {GUARD_BYTE} for b in got)


def test_no_blocks_returns():
    named = mixed_blocks()[:8]
    launch = Launch([(run, raw_len, i) for i, (_, run, raw_len, _, _) in enumerate(named)])
    got, err = launch.run(nblock=0)
    assert err == [-1] * 8
    assert all(set(b) == {GUARD_BYTE} for b in got)
