"""GPU tests of frame discovery (csrc/hip/kernels.hip
frame_scan_pass_kernel<COUNT|EMIT>, frame_chain_kernel) against the
every-position reference of frame_scan_cases.py: the emitted candidate list
itself, not only the frames that survive the chain check. Integers only,
compared exactly."""

import numpy as np
import pytest

import frame_scan_cases as F
from spark_tfrecord_amd import _native

pytestmark = pytest.mark.gpu

GUARD = 64  # untouched words behind every output array


def _g():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _to_device(img: bytes):
    import torch
    # a fresh allocation: 8-byte aligned, as the kernel's word loads need
    return torch.from_numpy(np.frombuffer(img, np.uint8).copy()).cuda()


def _device_candidates(data, N, ranges):
    """COUNT per range into one block array, prefix sum, EMIT per range
    into one candidate array: what _emit_and_chain does. Returns the block
    counts of each range and the candidates."""
    import torch
    g = _g()
    nb = [int(_native.gpu_frame_scan_blocks(s, e)) for s, e in ranges]
    B = sum(nb)
    counts = torch.full((B + GUARD,), -7, dtype=torch.int64, device="cuda")
    base = 0
    for (s, e), n in zip(ranges, nb):
        _native.gpu_frame_scan_count(data.data_ptr(), N, s, e, base,
                                     counts.data_ptr(), g._stream())
        base += n
    assert (counts[B:] == -7).all()
    block_off = g.excl_sum(counts[:B])
    C = int(block_off[-1].item())
    pos = torch.full((C + GUARD,), -1, dtype=torch.int64, device="cuda")
    lens = torch.full((C + GUARD,), -1, dtype=torch.int64, device="cuda")
    base = 0
    for (s, e), n in zip(ranges, nb):
        _native.gpu_frame_scan_emit(data.data_ptr(), N, s, e, base,
                                    block_off.data_ptr(), pos.data_ptr(),
                                    lens.data_ptr(), g._stream())
        base += n
    pos, lens = pos.cpu().numpy(), lens.cpu().numpy()
    assert (pos[C:] == -1).all() and (lens[C:] == -1).all()
    per_range = np.split(counts[:B].cpu().numpy(), np.cumsum(nb)[:-1])
    return per_range, pos[:C], lens[:C]


def _check_candidates(img: bytes, N: int, ranges, tag):
    per_range, pos, lens = _device_candidates(_to_device(img), N, ranges)
    want_pos, want_len = F.ref_candidates(img[:N], ranges)
    for (s, e), counts in zip(ranges, per_range):
        n = int(((want_pos >= s) & (want_pos < e)).sum())
        assert int(counts.sum()) == n, (tag, s, e)
    assert np.array_equal(pos, want_pos), tag
    assert np.array_equal(lens, want_len), tag


# ---------------------------------------------------------------------------
# 1. candidates
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(F.CASES))
def test_candidates(name):
    img = F.CASES[name].img
    for key, ranges in F.range_sets(name).items():
        _check_candidates(img, len(img), ranges, (name, key))


@pytest.mark.parametrize("name", list(F.GARBAGE))
def test_candidates_of_garbage(name):
    img = F.GARBAGE[name]
    per_range, pos, _ = _device_candidates(_to_device(img), len(img),
                                           [(0, len(img))])
    assert sum(int(c.sum()) for c in per_range) == 0 and pos.size == 0


@pytest.mark.parametrize("name", F.TAIL_CASES)
def test_tail_branch_equals_word_branch(name):
    # With 32 zero bytes behind it, every chunk of the file takes the
    # full-word loads; alone, its last chunks are assembled byte by byte.
    # Both equal the reference over the same positions, and the reference
    # is the same for both (test_frame_scan_cases.py).
    img = F.CASES[name].img
    N = len(img)
    _check_candidates(img, N, [(0, N)], (name, "tail"))
    _check_candidates(img + bytes(F.PAD), N + F.PAD, [(0, N)], (name, "word"))
    _check_candidates(img + bytes(F.PAD), N + F.PAD, [(0, N + F.PAD)],
                      (name, "word, padding scanned"))


# ---------------------------------------------------------------------------
# 2. chain kernel
# ---------------------------------------------------------------------------

# grid_for caps the grid at 8192 blocks of 256: only more candidates than
# that take the grid-stride loop a second time
CHAIN_SIZES = (1, 255, 256, 257, 70000, 8192 * 256 + 257)
CARRY_IN = 123457


def _run_chain(pos, lens, carry_in):
    import torch
    g = _g()
    C = len(pos)
    d_pos = torch.as_tensor(pos, device="cuda")
    d_len = torch.as_tensor(lens, device="cuda")
    # carry_in, carry_out, broken: three words of one block, as the
    # streamed read keeps them
    words = torch.tensor([carry_in, -99, 0], dtype=torch.int64, device="cuda")
    off = torch.full((C + GUARD,), -1, dtype=torch.int64, device="cuda")
    p = words.data_ptr()
    _native.gpu_frame_chain(d_pos.data_ptr(), d_len.data_ptr(), C, p, p + 8,
                            off.data_ptr(), p + 16, g._stream())
    w = words.cpu().numpy()
    off = off.cpu().numpy()
    assert (off[C:] == -1).all() and w[0] == carry_in
    return off[:C], int(w[1]), int(w[2])


@pytest.mark.parametrize("C", CHAIN_SIZES)
def test_chain_kernel(C):
    cases = F.chain_cases(C, CARRY_IN)
    assert {"clean", "first", "last"} <= set(cases)
    assert ("block_edge" in cases) == (C > 256)
    for name, (pos, lens) in cases.items():
        want_off, want_carry, want_broken = F.ref_chain(pos, lens, CARRY_IN)
        assert want_broken == (name != "clean")
        off, carry, broken = _run_chain(pos, lens, CARRY_IN)
        assert np.array_equal(off, want_off), name
        assert carry == want_carry, name
        assert broken == int(want_broken), name
    # the same candidates after another chain end: link 0 alone breaks
    pos, lens = cases["clean"]
    assert _run_chain(pos, lens, CARRY_IN + 1)[1:] == (
        F.ref_chain(pos, lens, CARRY_IN + 1)[1], 1)


def test_chain_kernel_no_candidates_leaves_carry_out():
    z = np.zeros(0, np.int64)
    off, carry, broken = _run_chain(z, z, CARRY_IN)
    assert F.ref_chain(z, z, CARRY_IN)[1] is None
    assert off.size == 0 and carry == -99 and broken == 0


# ---------------------------------------------------------------------------
# 3. scan_frames_device as a whole
# ---------------------------------------------------------------------------

def _cpu_walk(img: bytes):
    off, lens = _native.scan_frames(np.frombuffer(img, np.uint8), True)
    return np.asarray(off, np.int64), np.asarray(lens, np.int64)


@pytest.mark.parametrize("name", list(F.CASES))
def test_scan_frames_device(name):
    case = F.CASES[name]
    g = _g()
    if case.torn:
        with pytest.raises(RuntimeError, match="broken frame chain"):
            g.scan_frames_device(_to_device(case.img))
        return
    # decoy images come through the host stitch
    off, lens = g.scan_frames_device(_to_device(case.img))
    want_off, want_len = _cpu_walk(case.img)
    assert np.array_equal(off.cpu().numpy(), want_off)
    assert np.array_equal(lens.cpu().numpy(), want_len)


@pytest.mark.parametrize("name", list(F.GARBAGE))
def test_scan_frames_device_garbage(name):
    with pytest.raises(RuntimeError, match="no valid frame header found"):
        _g().scan_frames_device(_to_device(F.GARBAGE[name]))


def test_scan_frames_device_empty():
    import torch
    off, lens = _g().scan_frames_device(
        torch.zeros(0, dtype=torch.uint8, device="cuda"))
    assert off.numel() == 0 and lens.numel() == 0
    assert off.dtype == lens.dtype == torch.int64
