"""GPU tests of the segmented-gzip inflater (csrc/hip/inflate.hip): the cases
of tests/inflate_cases.py through all three kernels (whole-wave, half-wave
pairs, quarter-wave with 9/7-bit root tables) against zlib, then through
`_device_inflate_group` as files. The lane-split copies, the lane-strided
table fill and the fences between them exist only on the device; the CPU
tier (test_inflate_core.py) ran the same cases through the serial build
first. Malformed segments must come back as error words, and nothing may be
written outside a segment's own output range."""

import os

import numpy as np
import pytest

import inflate_cases as C
import spark_tfrecord_amd as stf
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P

pytestmark = pytest.mark.gpu

VALID = C.valid_segments()
MALFORMED = C.malformed_segments()
BY_NAME = {n: (c, w) for n, c, w in VALID}
MODES = [1, 2, 4]
STREAMS_PER_BLOCK = {1: 4, 2: 8, 4: 16}  # 256 threads / 64, 32, 16 lanes
FILL = 0xEE
GAP = 64


def _gpu_engine():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _launch(segs, mode):
    """One launch over [(comp, expect_len)]: every segment's output in its
    own slice of a buffer of FILL, GAP bytes of FILL around each. Returns
    (error word, the buffer as numpy, [each slice's offset])."""
    import torch

    g = _gpu_engine()
    in_len = np.array([len(c) for c, _ in segs], np.int64)
    out_len = np.array([n for _, n in segs], np.int64)
    in_off = np.concatenate([[0], np.cumsum(in_len)[:-1]])
    out_off = GAP + np.concatenate([[0], np.cumsum(out_len + GAP)[:-1]])
    total = int(out_off[-1] + out_len[-1] + GAP)
    blob = b"".join(c for c, _ in segs)
    comp = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).cuda()
    meta = torch.as_tensor(np.stack([in_off, in_len, out_off, out_len])).cuda()
    data = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    err = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    _native.gpu_inflate_segments(
        comp.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(),
        meta[2].data_ptr(), meta[3].data_ptr(), len(segs), data.data_ptr(),
        err.data_ptr(), g._stream(), mode)
    torch.cuda.synchronize()
    return int(err.item()), data.cpu().numpy(), out_off.tolist()


def _check(buf, offs, wants, what):
    """Every slice with bytes in `wants` equals them (None = a refused
    segment's slice, contents free), and every byte between slices is
    still FILL."""
    expect = np.full(buf.size, FILL, np.uint8)
    known = np.ones(buf.size, bool)
    for off, (name, want, n) in zip(offs, wants):
        if want is None:
            known[off:off + n] = False
        else:
            expect[off:off + n] = np.frombuffer(want, np.uint8)
    bad = np.nonzero(known & (buf != expect))[0]
    if bad.size:
        pos = int(bad[0])
        k = int(np.searchsorted(offs, pos, side="right")) - 1
        name, _, n = wants[max(k, 0)]
        where = "inside" if k >= 0 and pos < offs[k] + n else "in the gap after"
        raise AssertionError(
            f"{what}: {bad.size} wrong bytes, the first at buffer byte {pos}, "
            f"{where} segment {k} ({name}) at its byte {pos - offs[max(k, 0)]}")


def _ordered(order):
    segs = list(VALID)
    if order == "reversed":
        segs.reverse()
    elif order == "odd":
        segs = segs[1:] if len(segs) % 2 == 0 else segs[2:]
    elif order == "shuffled":
        segs = [segs[i] for i in
                np.random.default_rng(5).permutation(len(segs))]
    return segs


@pytest.mark.parametrize("order", ["forward", "reversed", "odd", "shuffled"])
@pytest.mark.parametrize("mode", MODES)
def test_valid_segments_in_one_launch(mode, order):
    segs = _ordered(order)
    assert (len(segs) % 2 == 1) == (order == "odd")
    # neighbours share a wave in modes 2 and 4: they differ in kind
    kinds = [n.split("_")[0] for n, _, _ in segs]
    mixed = sum(a != b for a, b in zip(kinds[::2], kinds[1::2]))
    assert mixed >= (20 if order == "shuffled" else 2)
    err, buf, offs = _launch([(c, len(w)) for _, c, w in segs], mode)
    assert err == -1, (f"segment {(err >> 8) - 1} "
                       f"({segs[(err >> 8) - 1][0]}), cause {err & 0xFF}")
    _check(buf, offs, [(n, w, len(w)) for n, _, w in segs],
           f"mode {mode}, {order}")


NEIGHBOURS = ["stored_after_3_literals_63_256", "long_len10_dist8",
              "long_len258_dist258", "fixed_literals_sync",
              "no_distance_code", "one_distance_code",
              "blocks_fixed_dyn_stored_dyn_sync", "end_of_block_only",
              "zlib_level6_text_seg1", "match_reads_stored_bytes",
              "zlib_huffman_only_wide_seg1", "long_len3_dist1"]


def _host_cause(comp, expect):
    cause = C.host_cause(comp, expect)
    assert cause != 0 and cause == C.host_cause(comp, expect, 9, 7)
    return cause


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("mode", MODES)
def test_malformed_segment_among_valid_ones(mode, where):
    good = [(n,) + BY_NAME[n] for n in NEIGHBOURS]
    index = {"first": 0, "middle": len(good) // 2 + 1, "last": len(good)}[where]
    for name, comp, expect, _ in MALFORMED:
        cause = _host_cause(comp, expect)
        segs = [(c, len(w)) for _, c, w in good]
        segs.insert(index, (comp, expect))
        wants = [(n, w, len(w)) for n, _, w in good]
        wants.insert(index, (name, None, expect))
        err, buf, offs = _launch(segs, mode)
        assert err == ((index + 1) << 8) | cause, \
            (name, (err >> 8) - 1, err & 0xFF, cause)
        _check(buf, offs, wants, f"mode {mode}, {name} {where}")


@pytest.mark.parametrize("mode", MODES)
def test_two_malformed_segments_name_the_lower_index(mode):
    good = [(n,) + BY_NAME[n] for n in NEIGHBOURS]
    bad = {m[0]: m for m in MALFORMED}
    a, b = bad["literal_past_output"], bad["block_type_3"]
    for first, second in ((a, b), (b, a)):
        segs = [(c, len(w)) for _, c, w in good]
        wants = [(n, w, len(w)) for n, _, w in good]
        for index, m in ((9, second), (2, first)):
            segs.insert(index, (m[1], m[2]))
            wants.insert(index, (m[0], None, m[2]))
        assert segs[2][0] == first[1] and segs[10][0] == second[1]
        err, buf, offs = _launch(segs, mode)
        assert err == (3 << 8) | _host_cause(first[1], first[2])
        _check(buf, offs, wants, f"mode {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_more_segments_than_resident_streams(mode):
    """cap * streams-per-block + 1000 copies of one small segment: the last
    1000 are reached only through the grid-stride loop."""
    import torch

    g = _gpu_engine()
    s = C.Stream().fixed(final=True).lits(b"grid-stride").match(6, 11)
    s.lits(b"+!?").end()
    comp, want = s.comp(), bytes(s.data)
    assert len(want) == 20 and C.zlib_inflate(comp)[0] == want
    n = _native.INFLATE_MAX_BLOCKS * STREAMS_PER_BLOCK[mode] + 1000
    dev = torch.frombuffer(bytearray(comp), dtype=torch.uint8).cuda()
    zeros = torch.zeros(n, dtype=torch.int64, device="cuda")
    in_len = torch.full((n,), len(comp), dtype=torch.int64, device="cuda")
    out_off = torch.arange(n, dtype=torch.int64, device="cuda") * 20 + GAP
    out_len = torch.full((n,), 20, dtype=torch.int64, device="cuda")
    data = torch.full((n * 20 + 2 * GAP,), FILL, dtype=torch.uint8,
                      device="cuda")
    err = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    _native.gpu_inflate_segments(
        dev.data_ptr(), zeros.data_ptr(), in_len.data_ptr(),
        out_off.data_ptr(), out_len.data_ptr(), n, data.data_ptr(),
        err.data_ptr(), g._stream(), mode)
    torch.cuda.synchronize()
    assert int(err.item()) == -1
    buf = data.cpu().numpy()
    assert (buf[:GAP] == FILL).all() and (buf[-GAP:] == FILL).all()
    rows = buf[GAP:-GAP].reshape(n, 20)
    wrong = np.nonzero((rows != np.frombuffer(want, np.uint8)).any(axis=1))[0]
    assert wrong.size == 0, (wrong.size, wrong[:5].tolist())


# ---------------------------------------------------------------------------
# files: _device_inflate_group and the reads built on it
# ---------------------------------------------------------------------------

def _segs(*names):
    return [BY_NAME[n] for n in names]


# ratios on both sides of the 0.85 the router splits at, sizes out of order
MIXED_FILES = [
    _segs("long_geometry_sync", "fixed_literals_sync",
          "zlib_level6_wide_seg0", "stored_after_5_literals_511_1000",
          "zlib_level9_text_seg0", "long_tail_4_literals"),
    _segs("zlib_huffman_only_wide_seg0", "zlib_rle_skewed_seg0",
          "zlib_fixed_wide_seg1"),
    _segs("empty_as_zlib_writes_it"),
    _segs("empty_sync_only", "stored_after_0_literals_1_257",
          "zlib_level1_wide_seg0", "one_distance_code"),
    _segs("stored_65535"),
]


def _write(tmp_path, name, blob):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(blob)
    return p


def _group(g, tmp_path, files):
    """Decode [gzip image] as one group, every file's output GAP bytes
    from the next in a buffer of FILL; (ok, buffer, [out_base])."""
    import torch

    items = []
    base = GAP
    for k, gz in enumerate(files):
        p = _write(tmp_path, f"part-{k:05d}.tfrecord.gz", gz)
        meta = g.gz_device_meta(p)
        assert meta == P.parse_gz_segments(gz)
        items.append((p, meta, base))
        base += meta[3] + GAP
    data = torch.full((base,), FILL, dtype=torch.uint8, device="cuda")
    ok = g._device_inflate_group(data, items, "cuda")
    return ok, data.cpu().numpy(), [it[2] for it in items]


def _spy_launches(monkeypatch):
    calls = []
    real = _native.gpu_inflate_segments

    def spy(*a):
        calls.append((a[9], a[5]))  # (streams_per_wave, segments)
        return real(*a)

    monkeypatch.setattr(_native, "gpu_inflate_segments", spy)
    return calls


@pytest.mark.parametrize("force", [None, "1", "2", "4"])
def test_mixed_group(tmp_path, monkeypatch, force):
    g = _gpu_engine()
    if force is None:
        monkeypatch.delenv("TFREC_INFLATE_STREAMS", raising=False)
    else:
        monkeypatch.setenv("TFREC_INFLATE_STREAMS", force)
    built = [C.gz_file(f) for f in MIXED_FILES]
    calls = _spy_launches(monkeypatch)
    ok, buf, bases = _group(g, tmp_path, [gz for gz, _ in built])
    assert ok is True
    _check(buf, bases, [(f"file {k}", d, len(d))
                        for k, (_, d) in enumerate(built)], f"force {force}")
    nseg = sum(len(f) for f in MIXED_FILES)
    if force is None:
        lit = sum(len(c) >= 0.85 * max(len(w), 1)
                  for f in MIXED_FILES for c, w in f)
        assert 2 < lit < nseg - 2
        assert calls == [(2, lit), (1, nseg - lit)]
        # the half-wave launch pairs by size: that order is not the files'
        sizes = [len(w) for f in MIXED_FILES for c, w in f
                 if len(c) >= 0.85 * max(len(w), 1)]
        assert sizes != sorted(sizes, reverse=True)
    else:
        assert calls == [(int(force), nseg)]


@pytest.mark.parametrize("kind,victim", [("literal", "fixed_literals_sync"),
                                         ("match", "long_geometry_sync")])
def test_flipped_bit_in_either_launch(tmp_path, monkeypatch, kind, victim):
    g = _gpu_engine()
    monkeypatch.delenv("TFREC_INFLATE_STREAMS", raising=False)
    comp, want = BY_NAME[victim]
    assert (len(comp) >= 0.85 * len(want)) == (kind == "literal")
    bad = C.flip_bit_refused(comp, len(want))
    assert C.host_cause(bad, len(want)) != 0
    built = [C.gz_file(f) for f in MIXED_FILES]
    # a damaged file would fail gz_file's own zlib check: take the good
    # image and flip the same bit in it
    good0, data0 = built[0]
    at = good0.index(comp)
    img0 = good0[:at] + bad + good0[at + len(comp):]
    assert len(img0) == len(good0) and good0.count(comp) == 1
    built[0] = (img0, data0)
    calls = _spy_launches(monkeypatch)
    ok, buf, bases = _group(g, tmp_path, [gz for gz, _ in built])
    assert ok is False
    assert [c[0] for c in calls] == [2, 1]
    # the other files are whole, and nothing left its slice
    _check(buf, bases, [("file 0", None, len(data0))] +
           [(f"file {k}", d, len(d)) for k, (_, d) in enumerate(built)
            if k], kind)
    p = _write(tmp_path, "alone.tfrecord.gz", img0)
    assert g.read_gzip_file_to_device(p) is None
    assert g.read_gzip_file_to_device(
        _write(tmp_path, "whole.tfrecord.gz", good0)) is not None


def _outcome(path, engine):
    try:
        df = stf.read_tfrecord(path, record_type="ByteArray", engine=engine)
        return "rows", [r["byteArray"] for r in df.collect()]
    except Exception as e:  # noqa: BLE001 - whatever the engine raises
        return "error", type(e).__name__, str(e)


def test_read_of_a_dataset_with_a_damaged_file(tmp_path):
    """A bit flipped inside a frame's payload, in a segment of Huffman-coded
    literals: the device refuses the file, the host codec then says what
    the CPU engine says of it."""
    import pyarrow as pa

    g = _gpu_engine()
    rng = np.random.default_rng(21)
    payloads = [bytes(rng.integers(0, 200, 300).astype(np.uint8))
                for _ in range(900)]
    raws = []
    for k in range(3):
        d = str(tmp_path / f"src{k}")
        t = pa.table({"byteArray": pa.array(payloads[300 * k:300 * k + 300],
                                            type=pa.large_binary())})
        stf.write_tfrecord(t, d, record_type="ByteArray", engine="cpu")
        (f,) = P.list_data_files(d)
        with open(f, "rb") as fh:
            raws.append(fh.read())
    out = tmp_path / "data"
    out.mkdir()
    for k in (0, 2):
        _write(out, f"part-0000{k}.tfrecord.gz",
               P.compress_bytes(raws[k], "gzip"))
    segs = C.cut_like_compress_bytes(raws[1], 6, 0)
    assert len(segs) >= 3
    assert all(len(c) >= 0.85 * len(w) and len(c) < 0.98 * len(w)
               for c, w in segs)
    good, _ = C.gz_file(segs)
    assert good == P.compress_bytes(raws[1], "gzip")
    mid = _write(out, "part-00001.tfrecord.gz", good)
    assert _outcome(str(out), "cpu") == ("rows", payloads)
    assert _outcome(str(out), "gpu") == ("rows", payloads)
    comp, want = segs[1]
    bad = C.flip_bit_refused(comp, len(want))
    bit = next(i for i in range(len(comp)) if comp[i] != bad[i])
    assert bit > 100  # past the block header: among the payload's literals
    at = good.index(comp)
    _write(out, "part-00001.tfrecord.gz",
           good[:at] + bad + good[at + len(comp):])
    assert g.read_gzip_file_to_device(mid) is None
    cpu = _outcome(str(out), "cpu")
    assert cpu[0] == "error"
    assert _outcome(str(out), "gpu") == cpu
