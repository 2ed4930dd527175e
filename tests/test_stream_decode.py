"""Streamed pipelined read vs the unstreamed decode on the same bytes.

read_file_to_batch_pipelined discovers, chain-checks, scans and extracts each
H2D slice's records while later slices are in flight; the oracle is
decode_device(scan_frames_device(...)) over the whole image. No arithmetic
is involved, so every array of every column must match with torch.equal, and
every error must carry the same type and message (record index included).
Shapes are small: _READ_SLICE is patched down to a few KiB so that a file of
tens of KB already spans many slices.
"""

import struct

import numpy as np
import pytest

import spark_tfrecord_amd as stf
from spark_tfrecord_amd.columnar import RecordBatch, column_from_values
from spark_tfrecord_amd.engine import cpu as cpu_engine

pytestmark = pytest.mark.gpu

PARTS = ("presence", "row_off", "values", "elem_off", "list_off", "sub_off")


def _g():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _batch(schema, columns):
    n = len(next(iter(columns.values())))
    cols = [column_from_values(columns[f.name], f.dataType, True, f.name)
            for f in schema.fields]
    return RecordBatch(schema, cols, n)


def _flagship(rows=300, seed=5):
    from bench import make_batch
    b = make_batch(rows, seed=seed)
    return cpu_engine.encode_batch(b, "Example"), b.schema, "Example"


def _ragged(n=400, seed=1):
    rng = np.random.default_rng(seed)
    schema = stf.StructType([
        stf.StructField("id", stf.LongType(), True),
        stf.StructField("s", stf.StringType(), True),
        stf.StructField("arr", stf.ArrayType(stf.LongType()), True),
        stf.StructField("farr", stf.ArrayType(stf.FloatType()), True),
        stf.StructField("blobs", stf.ArrayType(stf.BinaryType()), True),
    ])
    img = cpu_engine.encode_batch(_batch(schema, {
        "id": [int(v) if i % 5 else None
               for i, v in enumerate(rng.integers(-2**60, 2**60, n))],
        "s": [f"name-{i}" * (i % 4) if i % 7 else None for i in range(n)],
        "arr": [list(rng.integers(-100, 100, i % 5)) for i in range(n)],
        "farr": [list(rng.random(i % 8).astype(float)) for i in range(n)],
        "blobs": [[bytes(rng.integers(0, 256, int(k), dtype=np.uint8))
                   for k in rng.integers(0, 40, i % 3)] for i in range(n)],
    }), "Example")
    # decode with a field the file never carries
    schema = stf.StructType(list(schema.fields) + [
        stf.StructField("absent", stf.ArrayType(stf.FloatType()), True)])
    return img, schema, "Example"


def _sequence(n=300, seed=4):
    rng = np.random.default_rng(seed)
    schema = stf.StructType([
        stf.StructField("ctx", stf.LongType(), True),
        stf.StructField("rag", stf.ArrayType(stf.ArrayType(stf.FloatType())), True),
        stf.StructField("toks", stf.ArrayType(stf.ArrayType(stf.StringType())), True),
    ])
    img = cpu_engine.encode_batch(_batch(schema, {
        "ctx": [int(v) for v in rng.integers(0, 10, n)],
        "rag": [[list(rng.random(rng.integers(0, 4)).astype(float))
                 for _ in range(rng.integers(0, 3))] for _ in range(n)],
        "toks": [[[f"t{i}-{j}" for j in range(i % 3)] for _ in range(i % 4)]
                 for i in range(n)],
    }), "SequenceExample")
    return img, schema, "SequenceExample"


_S = stf.StructType([stf.StructField("s", stf.StringType(), True)])


def _strings(lengths):
    return cpu_engine.encode_batch(
        _batch(_S, {"s": ["x" * int(k) for k in lengths]}), "Example")


def _frames_of(nbytes, count):
    """`count` one-string records whose frames are exactly nbytes each."""
    for k in range(nbytes):
        if len(_strings([k])) == nbytes:
            return _strings([k] * count)
    raise AssertionError(f"no string length frames to {nbytes} bytes")


def _frame_bounds(img):
    from spark_tfrecord_amd import _native
    off, lens = _native.scan_frame_headers(np.frombuffer(img, np.uint8))
    return np.asarray(off), np.asarray(lens)


def _outcome(fn):
    try:
        return fn()
    except Exception as e:  # compared by type and full message below
        return (type(e), str(e))


def _oracle(img, schema, record_type, verify_crc):
    import torch
    g = _g()

    def run():
        data = torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda() \
            if len(img) else torch.zeros(0, dtype=torch.uint8, device="cuda")
        off, lens = g.scan_frames_device(data)
        return g.decode_device(data, off, lens, schema, record_type, verify_crc)
    return _outcome(run)


def _streamed(tmp_path, monkeypatch, img, schema, record_type, verify_crc,
              read_slice, extract=True):
    from spark_tfrecord_amd import _native
    g = _g()
    path = str(tmp_path / "f.tfrecord")
    with open(path, "wb") as f:
        f.write(img)
    if img:  # the streamed reader needs the registered mapping
        assert _native.file_mmap_pinned(path, len(img), False)[1]
    monkeypatch.setattr(g, "_STREAM_DECODE", True)
    monkeypatch.setattr(g, "_STREAM_EXTRACT", extract)
    if read_slice:
        monkeypatch.setattr(g, "_READ_SLICE", read_slice)
    g.last_read.clear()
    return _outcome(lambda: g.read_file_to_batch_pipelined(
        path, schema, record_type, verify_crc=verify_crc))


def _assert_same(got, want):
    import torch
    if isinstance(want, tuple):
        assert got == want
        return
    assert not isinstance(got, tuple), got
    assert got.num_rows == want.num_rows
    for f, a, b in zip(want.schema.fields, got.columns, want.columns):
        assert (a.kind, a.is_seq) == (b.kind, b.is_seq)
        for part in PARTS:
            ta, tb = getattr(a, part), getattr(b, part)
            assert (ta is None) == (tb is None), (f.name, part)
            if tb is not None:
                assert ta.dtype == tb.dtype and torch.equal(ta, tb), \
                    (f.name, part)


def _assert_matches_host_codec(want, img, schema, record_type, verify_crc):
    """The oracle shares its extraction and column assembly with the code
    under test, so it is itself anchored to the host codec."""
    host = cpu_engine.decode_buffer(np.frombuffer(img, np.uint8), schema,
                                    record_type, verify_crc)
    dev = _g().batch_to_host(want)
    assert dev.num_rows == host.num_rows
    assert len(dev.columns) == len(host.columns)
    for f, a, b in zip(schema.fields, dev.columns, host.columns):
        for part in PARTS:
            va, vb = getattr(a, part), getattr(b, part)
            assert (va is None) == (vb is None), (f.name, part)
            if vb is not None:
                assert np.array_equal(np.asarray(va), np.asarray(vb)), \
                    (f.name, part)


def _check(tmp_path, monkeypatch, case, read_slice, verify_crc, extract,
           path="streamed", min_slices=1):
    img, schema, record_type = case
    want = _oracle(img, schema, record_type, verify_crc)
    # The empty file stays un-anchored: decode_device's empty batch carries no
    # elem_off where the host codec returns [0] (a difference older than
    # this check).
    if not isinstance(want, tuple) and img:
        _assert_matches_host_codec(want, img, schema, record_type, verify_crc)
    got = _streamed(tmp_path, monkeypatch, img, schema, record_type,
                    verify_crc, read_slice, extract)
    _assert_same(got, want)
    g = _g()
    if img:
        assert g.last_read["path"] == path
        assert g.last_read["slices"] >= min_slices
    return want


crc = pytest.mark.parametrize("verify_crc", [True, False])
ext = pytest.mark.parametrize("extract", [True, False])


@crc
@ext
@pytest.mark.parametrize("read_slice,min_slices", [(16 << 10, 4), (2 << 10, 21)])
def test_flagship_shape(tmp_path, monkeypatch, verify_crc, extract, read_slice,
                        min_slices):
    # 2 KiB slices: more than 20 slices, so carries accumulate
    want = _check(tmp_path, monkeypatch, _flagship(), read_slice, verify_crc,
                  extract, min_slices=min_slices)
    assert want.num_rows == 300


@crc
@ext
def test_whole_slices_alternating_between_the_streams(tmp_path, monkeypatch,
                                                      verify_crc, extract):
    monkeypatch.setattr(_g(), "_SPLIT_SLICES", False)
    _check(tmp_path, monkeypatch, _flagship(), 4 << 10, verify_crc, extract,
           min_slices=15)


def test_forced_unstreamed_path(tmp_path, monkeypatch):
    g = _g()
    img, schema, rt = _flagship()
    want = _oracle(img, schema, rt, True)
    path = str(tmp_path / "u.tfrecord")
    with open(path, "wb") as f:
        f.write(img)
    monkeypatch.setattr(g, "_STREAM_DECODE", False)
    monkeypatch.setattr(g, "_READ_SLICE", 8 << 10)
    _assert_same(g.read_file_to_batch_pipelined(path, schema, rt), want)
    assert g.last_read["path"] == "unstreamed"


def test_whole_file_decode_allocates_exactly():
    # decode_device knows every total before it allocates: the growable value
    # buffers it shares with the streamed read must not add headroom there
    import torch
    g = _g()
    img, schema, rt = _flagship()
    data = torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda()
    off, lens = g.scan_frames_device(data)
    batch = g.decode_device(data, off, lens, schema, rt, True)
    assert batch.num_rows == 300
    checked = 0
    for f, c in zip(schema.fields, batch.columns):
        for part in ("values", "elem_off", "sub_off"):
            t = getattr(c, part)
            if t is not None:
                assert t.untyped_storage().nbytes() == \
                    t.numel() * t.element_size(), (f.name, part)
                checked += 1
    assert checked >= len(batch.columns)


@crc
@ext
def test_ragged_example(tmp_path, monkeypatch, verify_crc, extract):
    _check(tmp_path, monkeypatch, _ragged(), 8 << 10, verify_crc, extract,
           min_slices=4)


@crc
@ext
def test_sequence_example(tmp_path, monkeypatch, verify_crc, extract):
    want = _check(tmp_path, monkeypatch, _sequence(), 4 << 10, verify_crc,
                  extract, min_slices=4)
    assert want.columns[1].list_off is not None
    assert want.columns[1].sub_off is not None


@crc
@ext
@pytest.mark.parametrize("odd_prefix", [False, True])
def test_records_end_on_slice_boundaries(tmp_path, monkeypatch, verify_crc,
                                         extract, odd_prefix):
    # 256-byte frames, 4096-byte slices: every 16th record ends exactly on a
    # boundary. With an odd-sized first record the frame headers straddle
    # the boundaries instead (the 32-byte deferral).
    img = _frames_of(256, 64)
    if odd_prefix:
        # a 250-byte first frame puts a frame header at 4096 j - 6
        img = _frames_of(250, 1) + img
        off, _ = _frame_bounds(img)
        assert 4096 - 6 in (off - 12)
    _check(tmp_path, monkeypatch, (img, _S, "Example"), 4096, verify_crc,
           extract, min_slices=4)


@crc
@ext
def test_slice_smaller_than_a_record(tmp_path, monkeypatch, verify_crc, extract):
    # ~6 KB records, 4 KiB slices: some slices complete no record at all
    img = _strings([6000 + 7 * i for i in range(12)])
    _check(tmp_path, monkeypatch, (img, _S, "Example"), 4 << 10, verify_crc,
           extract, min_slices=15)


@crc
@ext
def test_wave_kernels_with_straddling_records(tmp_path, monkeypatch, verify_crc,
                                              extract):
    # 12 KB records select the one-record-per-wave kernels; 16 KiB slices
    img = _strings([12_000 + 11 * i for i in range(40)])
    _check(tmp_path, monkeypatch, (img, _S, "Example"), 16 << 10, verify_crc,
           extract, min_slices=20)


@crc
@ext
@pytest.mark.parametrize("shape", ["below_one_slice", "one_record", "empty"])
def test_boundary_sizes(tmp_path, monkeypatch, verify_crc, extract, shape):
    img, schema, rt = _flagship(rows=50)
    if shape == "one_record":
        img, schema, rt = _flagship(rows=1)
    elif shape == "empty":
        img = b""
    want = _check(tmp_path, monkeypatch, (img, schema, rt), 0, verify_crc,
                  extract)
    assert want.num_rows == {"below_one_slice": 50, "one_record": 1,
                             "empty": 0}[shape]


@crc
@ext
def test_density_jump_regrows(tmp_path, monkeypatch, verify_crc, extract):
    # a few large records in the first slice, many tiny ones after it: with
    # no headroom the first estimate is far too small and the buffers regrow
    g = _g()
    monkeypatch.setattr(g, "_STREAM_HEADROOM", 1.0)
    img = _strings([3000, 3000, 3000] + [i % 5 for i in range(600)])
    _check(tmp_path, monkeypatch, (img, _S, "Example"), 4 << 10, verify_crc,
           extract, min_slices=6)
    assert g.last_read["regrows"] >= 1


def test_ranged_stat_scans_equal_one_full_call():
    import torch
    from spark_tfrecord_amd import _native
    g = _g()
    R, F, r1 = 1000, 3, 377  # r1 lies inside every field's segment
    stats = torch.randint(0, 1000, (R, F, 6), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def planes(stride):
        out = [torch.full((F, stride), -7, dtype=torch.int64, device="cuda")
               for _ in range(3)]
        for t in out:
            t[:, 0] = 0
        return out

    def scan(out, r0, r1, stride):
        ws = g._stat_scan_workspace(r1 - r0, F, stats.device)
        _native.gpu_stat_scans(ws.data_ptr(), ws.numel(), stats.data_ptr(),
                               R, F, *[t.data_ptr() for t in out], stream,
                               r0=r0, r1=r1, stride=stride)

    full = planes(R + 1)
    _native.gpu_stat_scans(
        g._stat_scan_workspace(R, F, stats.device).data_ptr(),
        g._stat_scan_workspace(R, F, stats.device).numel(), stats.data_ptr(),
        R, F, *[t.data_ptr() for t in full], stream)
    for k, t in enumerate(full):  # the full call against torch.cumsum
        assert torch.equal(t[:, 1:], stats[:, :, 2 + k].t().cumsum(1))
    stride = R + 1 + 50  # wider planes, as the streamed reader's are
    two = planes(stride)
    scan(two, 0, r1, stride)
    scan(two, r1, R, stride)
    for a, b in zip(two, full):
        assert torch.equal(a[:, :R + 1], b)
        assert bool((a[:, R + 1:] == -7).all())  # nothing past row R


def _flip(img, at):
    b = bytearray(img)
    b[at] ^= 0x5A
    return bytes(b)


@crc
@ext
@pytest.mark.parametrize("where", ["first", "middle", "last", "straddle"])
def test_flipped_payload_byte(tmp_path, monkeypatch, verify_crc, extract, where):
    img, schema, rt = _flagship()
    off, lens = _frame_bounds(img)
    span = 8 << 10
    if where == "straddle":
        cut = 3 * span
        k = int(np.nonzero((off < cut) & (off + lens > cut))[0][0])
    else:
        k = {"first": 3, "middle": 150, "last": 298}[where]
    # the last payload byte belongs to a value, not to the structure
    bad = _flip(img, int(off[k] + lens[k] - 1))
    want = _check(tmp_path, monkeypatch, (bad, schema, rt), span, verify_crc,
                  extract)
    if verify_crc:
        assert want == (RuntimeError, f"corrupt TFRecord: bad CRC in record {k}")


def _kind_mismatch_file():
    sf = stf.StructType([stf.StructField("v", stf.ArrayType(stf.FloatType()), True)])
    sl = stf.StructType([stf.StructField("v", stf.ArrayType(stf.LongType()), True)])
    good = cpu_engine.encode_batch(_batch(sf, {
        "v": [[float(i), 0.5] * 20 for i in range(300)]}), "Example")
    wrong = cpu_engine.encode_batch(_batch(sl, {"v": [[1, 2, 3]]}), "Example")
    off, lens = _frame_bounds(good)
    cut = int(off[10] - 12)  # start of frame 10
    return good[:cut] + wrong + good[cut:], sf, len(wrong)


@crc
@ext
def test_early_kind_mismatch_and_later_bad_crc(tmp_path, monkeypatch, verify_crc,
                                               extract):
    img, schema, shift = _kind_mismatch_file()
    off, lens = _frame_bounds(img)
    bad = _flip(img, int(off[200] + lens[200] - 1))  # inside a float value
    want = _check(tmp_path, monkeypatch, (bad, schema, "Example"), 4 << 10,
                  verify_crc, extract)
    assert want[0] is RuntimeError
    # the CRC verdict wins when CRCs are verified; the kind mismatch in
    # record 10 is reported otherwise
    assert ("bad CRC in record 200" in want[1]) == verify_crc
    assert ("record 10 " in want[1]) == (not verify_crc)


@crc
@ext
def test_truncated_mid_record(tmp_path, monkeypatch, verify_crc, extract):
    img, schema, rt = _flagship()
    want = _check(tmp_path, monkeypatch, (img[:-37], schema, rt), 8 << 10,
                  verify_crc, extract, path="fallback")
    assert want[0] is RuntimeError and "broken frame chain" in want[1]


@crc
@ext
@pytest.mark.parametrize("at", [2, 120, 199])
def test_false_positive_header_falls_back(tmp_path, monkeypatch, verify_crc,
                                          extract, at):
    # a bytes value that embeds a complete, valid frame header (length plus
    # masked length CRC): frame discovery reports it as a candidate, the
    # chain check rejects it, and the whole-file path stitches it out. The
    # file is three 4 KiB slices long and record `at` puts the fake header in
    # the first, the middle and the last of them: the streamed loop leaves
    # for the fallback from its first slice, mid-loop and at the end.
    from spark_tfrecord_amd import _native
    head = struct.pack("<Q", 5)
    fake = head + struct.pack("<I", _native.masked_crc32c(head)) + b"y" * 40
    schema = stf.StructType([stf.StructField("b", stf.BinaryType(), True)])
    vals = [b"z" * (i % 50) for i in range(200)]
    vals[at] = fake
    img = cpu_engine.encode_batch(_batch(schema, {"b": vals}), "Example")
    off, _ = _frame_bounds(img)
    assert len(img) > 2 * 4096 and len(img) <= 3 * 4096
    assert int(off[at]) // 4096 == {2: 0, 120: 1, 199: 2}[at]
    want = _check(tmp_path, monkeypatch, (img, schema, "Example"), 4 << 10,
                  verify_crc, extract, path="fallback")
    assert want.num_rows == 200
