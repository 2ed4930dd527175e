"""CPU tier of the LZ4 decoder's differential tests: every case of
tests/lz4_cases.py is checked here before tests/test_gpu_lz4_kernel.py sends
it to the device. A valid block must come out the same four ways: played
forward by the builder, from the plain-Python reference, from pyarrow's
`lz4_raw`, and from the host build of csrc/lz4_core.h (in place and through
the staging window, with exact and with spare room). A malformed block must
be refused by the reference and by the core, with the cause stated by hand;
a mutant's fate is the reference's."""

import re
import struct

import pytest

import lz4_cases as C
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P

RAW = {"match_sweep": C.match_sweep(), "literal_sweep": C.literal_sweep(),
       "window_edges": C.window_edges(), "encoder_streams": C.encoder_streams()}
CHUNKED = C.chunked()
BAD = C.malformed()
BAD_CONTAINERS = C.malformed_containers()
MUTANTS = C.mutants()


def host_block(comp, cap, window):
    """(bytes, 0) or (None, cause) of the host core."""
    try:
        return _native.host_unlz4_block(comp, cap, window), 0
    except RuntimeError as e:
        assert "cause" in str(e), e
        return None, int(str(e).rsplit(" ", 1)[1])


def host_container(tmp_path, block, raw_len, causes=None):
    """P.decompress_file of the one-block file image, or None; a refusal
    that names the core's cause appends it to `causes`."""
    p = tmp_path / "case.tfrecord.lz4"
    p.write_bytes(struct.pack(">I", raw_len) + block)
    try:
        return P.decompress_file(str(p))
    except ValueError as e:
        assert "lz4" in str(e), e
        m = re.search(r"cause (\d+)$", str(e))
        if m and causes is not None:
            causes.append(int(m.group(1)))
        return None


def mutant_causes():
    """{name: the host core's cause} of the mutants it refuses; the device
    must give the same."""
    return {name: host_block(comp, cap, True)[1]
            for name, comp, cap, want in MUTANTS if want is None}


def test_families_have_the_edges():
    names = [c[0] for f in RAW.values() for c in f]
    assert len(set(names)) == len(names)
    sizes = {f: (len(c), sum(len(x[1]) for x in c)) for f, c in RAW.items()}
    assert sizes["match_sweep"][0] > 1200 and sizes["literal_sweep"][0] == 23 * 64
    assert sum(n for _, n in sizes.values()) < 20 << 20
    we = dict((c[0], c[1]) for c in RAW["window_edges"])
    assert len(we["three_refills"]) > 3 * C.WINDOW
    assert len(C.encoder_streams()[-1][2]) == C.LZ4_MAX_BLOCK_RAW


@pytest.mark.parametrize("family", RAW)
def test_valid_blocks(family):
    for name, comp, want in RAW[family]:
        n = len(want)
        assert C.ref_decode(comp, n) == want, name
        assert C.ref_decode(comp, n + 77) == want, name
        assert C.LIB.decompress(comp, decompressed_size=n, asbytes=True) == want, name
        for window in (False, True):
            for cap in (n, n + 77):
                assert _native.host_unlz4_block(comp, cap, window) == want, (name, window, cap)
        # one byte less room, one byte less input: refused, by both
        assert C.ref_decode(comp, n - 1) is None, name
        assert C.ref_decode(comp[:-1], n) is None, name
        assert host_block(comp, n - 1, True)[1] == C.LZ_OUTPUT_OVERRUN, name
        assert host_block(comp[:-1], n, True)[1] in (C.LZ_LITERAL_PAST_INPUT,
                                                     C.LZ_INPUT_SHORT), name


@pytest.mark.parametrize("name,block,want", CHUNKED, ids=[c[0] for c in CHUNKED])
def test_container_blocks(tmp_path, name, block, want):
    assert C.ref_container(block, len(want)) == want
    assert host_container(tmp_path, block, len(want)) == want
    assert C.ref_container(block, len(want) + 1) is None
    assert C.ref_container(block, len(want) - 1) is None
    assert C.ref_container(block[:-1], len(want)) is None
    for _, comp, w in RAW["window_edges"][:3]:  # a raw case as a one-chunk block
        assert C.ref_container(C.one_chunk(comp), len(w)) == w


@pytest.mark.parametrize("name,comp,cap,cause", BAD, ids=[c[0] for c in BAD])
def test_malformed_blocks(tmp_path, name, comp, cap, cause):
    assert C.ref_decode(comp, cap) is None
    for window in (False, True):
        assert host_block(comp, cap, window) == (None, cause)
    assert C.ref_container(C.one_chunk(comp), cap) is None
    causes = []
    assert host_container(tmp_path, C.one_chunk(comp), cap, causes) is None
    assert causes == [cause]


@pytest.mark.parametrize("name,block,raw_len,cause", BAD_CONTAINERS,
                         ids=[c[0] for c in BAD_CONTAINERS])
def test_malformed_container_blocks(tmp_path, name, block, raw_len, cause):
    assert C.ref_container(block, raw_len) is None
    causes = []
    assert host_container(tmp_path, block, raw_len, causes) is None
    # a chunk the core refuses: the host names the core's cause; the chunk
    # walk's own causes (8..10) exist only in unlz4_container_block, which
    # csrc/tests/lz4_selftest.cpp and the GPU tier run
    assert causes == ([cause] if cause <= C.LZ_INPUT_LEFT else [])


def test_mutants():
    refused = accepted = 0
    causes = mutant_causes()
    for name, comp, cap, want in MUTANTS:
        for window in (False, True):
            got, cause = host_block(comp, cap, window)
            assert got == want, (name, window)
            if want is None:
                assert cause == causes[name] and 1 <= cause <= 7, (name, window)
        if want is None:
            refused += 1
        elif "_byte" in name:
            assert len(want) > 0, name  # a block of raw_len 0 is no block
            accepted += 1
    n = sum("_byte" in m[0] for m in MUTANTS)
    assert n == 8 * 32 and refused + accepted == n
    # both outcomes, from the reference alone (lz4_cases.MUTANT_SEED)
    assert refused >= n // 4 and accepted >= 1, (refused, accepted)
