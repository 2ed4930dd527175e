"""CPU self-checks of the frame-discovery reference in frame_scan_cases.py:
before any kernel is compared with it, the every-position reference must
agree with the CPU engine's own frame walk, find exactly the planted decoys
on top, and its CRC must be the project's."""

import numpy as np
import pytest

import frame_scan_cases as F
from spark_tfrecord_amd import _native


def _cpu_walk(img: bytes):
    off, lens = _native.scan_frames(np.frombuffer(img, np.uint8), True)
    return np.asarray(off, np.int64) - 12, np.asarray(lens, np.int64)


def test_table_crc_is_the_projects():
    assert F.crc32c(b"123456789") == 0xE3069283  # the CRC32C check value
    rng = np.random.default_rng(0)
    for n in (0, 1, 8, 12, 100):
        b = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        assert F.masked_crc(b) == _native.masked_crc32c(b)


@pytest.mark.parametrize("name", list(F.CASES))
def test_reference_finds_frames_and_planted_decoys(name):
    case = F.CASES[name]
    img, N = case.img, len(case.img)
    assert N <= 72 << 10
    # the frames, payload CRCs included, by the CPU engine's walk
    fpos, flens = _cpu_walk(img[:case.valid])
    wpos, wlens = case.frames()
    assert np.array_equal(fpos, wpos) and np.array_equal(flens, wlens)
    pos, lens = F.ref_candidates(img, [(0, N)])
    epos, elens = case.expected()
    assert np.array_equal(pos, epos), name
    assert np.array_equal(lens, elens), name
    assert len(pos) == len(fpos) + len(case.decoys)
    assert (np.diff(pos) > 0).all()
    for p, n in case.decoys:
        assert p not in set(fpos.tolist())
        assert n <= N - p - 16


@pytest.mark.parametrize("name", list(F.CASES))
def test_reference_ranges_partition_the_whole_scan(name):
    case = F.CASES[name]
    N = len(case.img)
    wpos, wlens = F.ref_candidates(case.img, [(0, N)])
    for key, ranges in F.range_sets(name).items():
        assert all(0 <= s < e <= N for s, e in ranges), key
        assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), key
        pos, lens = F.ref_candidates(case.img, ranges)
        inside = np.zeros(len(wpos), bool)
        for s, e in ranges:
            inside |= (wpos >= s) & (wpos < e)
        assert np.array_equal(pos, wpos[inside]), key
        assert np.array_equal(lens, wlens[inside]), key


def test_range_sets_split_off_16_and_inside_a_header():
    sets = F.range_sets("big")
    assert sets["split_odd"][0][1] == 4099 and sets["split_odd"][1][1] == 8200
    cut = sets["split_in_header"][0][1]
    pos, _ = F.CASES["big"].expected()
    assert cut - 5 in set(pos.tolist())
    assert [e - s for s, e in sets["one_byte"]] == [1, 1]
    assert sets["gaps"][-1][1] < len(F.CASES["big"].img)


@pytest.mark.parametrize("name", F.TAIL_CASES)
def test_padding_leaves_the_reference_unchanged(name):
    # what lets the GPU test pin the byte-wise tail branch to the word
    # branch: zero padding adds no candidate and changes none below N
    img = F.CASES[name].img
    N = len(img)
    a = F.ref_candidates(img, [(0, N)])
    b = F.ref_candidates(img + bytes(F.PAD), [(0, N)])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = F.ref_candidates(img + bytes(F.PAD), [(0, N + F.PAD)])
    assert np.array_equal(a[0], c[0])


def test_cull_case_plants_sit_on_the_edge():
    case = F.CASES["cull"]
    N = len(case.img)
    assert [n for p, n in case.decoys] == [N - p - 16 for p, _ in case.decoys]
    # the culled plants are in the image with a valid CRC all the same
    for length in (2 ** 63, 2 ** 64 - 1, 2 ** 63 + 5):
        assert case.img.count(F.header(length)) == 1


@pytest.mark.parametrize("name", list(F.GARBAGE))
def test_garbage_has_no_candidate(name):
    img = F.GARBAGE[name]
    assert F.ref_candidates(img, [(0, len(img))])[0].size == 0


def test_torn_cases_cover_every_garbage_length_class():
    torn = [k for k in F.CASES if F.CASES[k].torn]
    assert len(torn) == len(F.TAIL_SIZES) - 1
    for k in torn:
        c = F.CASES[k]
        assert 1 <= len(c.img) - c.valid <= 15 and c.valid >= 16


def test_ref_chain():
    off, carry, broken = F.ref_chain([7, 30], [7, 1], 7)
    assert off.tolist() == [19, 42] and carry == 47 and not broken
    assert F.ref_chain([7, 31], [7, 1], 7)[2]
    assert F.ref_chain([8, 31], [7, 1], 7)[2]
    assert F.ref_chain([], [], 5) [1] is None
    for C in (1, 255, 256, 257):
        for name, (pos, lens) in F.chain_cases(C, 1000).items():
            assert len(pos) == C
            want = np.concatenate([[1000], (pos + 16 + lens)[:-1]])
            assert int((pos != want).sum()) == (0 if name == "clean" else 1)
