"""GPU tests of the many-files-one-image read (engine/gpu.py
read_files_to_batch, _upload_files, _read_file_staged) against the CPU
engine decoding each file alone: where the file boundaries fall in the
image, every upload route, and the staged route with the stream busy, when
the copies out of the shared staging buffer run long after the host has
gone on to the next file."""

import os
import time

import numpy as np
import pytest

import frame_scan_cases as F
import spark_tfrecord_amd as stf
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.arrow_interop import batch_to_table
from spark_tfrecord_amd.columnar import RecordBatch, column_from_values
from spark_tfrecord_amd.engine import cpu as cpu_engine
from spark_tfrecord_amd.infer import byte_array_schema
from spark_tfrecord_amd.io import paths as P
from spark_tfrecord_amd.io.reader import infer_schema_of_paths

pytestmark = pytest.mark.gpu


def _g():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _put(path, blob):
    with open(path, "wb") as f:
        f.write(blob)
    return str(path)


def _register_nothing(monkeypatch):
    monkeypatch.setattr(_native, "file_mmap_pinned",
                        lambda path, n, writable: (0, False))


# ---------------------------------------------------------------------------
# Files whose boundaries fall where the image's chunks and blocks do not
# ---------------------------------------------------------------------------

EXAMPLE_SCHEMA = stf.StructType([
    stf.StructField("b", stf.BinaryType(), True),
    stf.StructField("v", stf.ArrayType(stf.FloatType()), True),
    stf.StructField("x", stf.LongType(), True),
])

# (records, where the file's end falls in the image: residue, modulus)
FILE_PLAN = [(0, None), (1, (1, 16)), (40, (7, 16)), (13, (8, 16)),
             (0, None), (7, (9, 16)), (25, (15, 16)), (31, (0, 4096)),
             (0, None)]


def _example_file(first_row: int, rows: int, pad: int) -> bytes:
    """`rows` Example records; the last one's bytes field carries `pad`
    more bytes, which moves the file's end."""
    ids = range(first_row, first_row + rows)
    bs = [b"r%d" % i * (i % 4) for i in ids]
    bs[-1] += b"p" * pad
    cols = [
        column_from_values(bs, stf.BinaryType(), True, "b"),
        column_from_values([[i * 0.5, i + 0.25] for i in ids],
                           stf.ArrayType(stf.FloatType()), True, "v"),
        column_from_values([i * 7 - 100 for i in ids], stf.LongType(), True,
                           "x"),
    ]
    return cpu_engine.encode_batch(RecordBatch(EXAMPLE_SCHEMA, cols, rows),
                                   "Example")


def _bytes_file(first_row: int, rows: int, pad: int) -> bytes:
    sizes = [(5 * i) % 37 for i in range(first_row, first_row + rows)]
    sizes[-1] += pad
    return b"".join(F.frame(F.filler(n, first_row + k))
                    for k, n in enumerate(sizes))


def _fit(make, start: int, residue: int, modulus: int) -> bytes:
    """make(pad) for the pad that ends the file at `residue` mod `modulus`
    in an image where it starts at `start`. A pad byte adds one byte, or
    two where a length varint grows, so the pad is near the gap."""
    gap = (residue - start - len(make(0))) % modulus
    for base in (gap, gap + modulus):
        for pad in range(max(0, base - 12), base + 1):
            blob = make(pad)
            if (start + len(blob)) % modulus == residue:
                return blob
    raise AssertionError("no pad fits")


def _planned_files(record_type: str):
    make = _example_file if record_type == "Example" else _bytes_file
    blobs = []
    start = row = 0
    for rows, end in FILE_PLAN:
        blob = b""
        if rows:
            blob = _fit(lambda pad: make(row, rows, pad), start, *end)
        blobs.append(blob)
        start += len(blob)
        row += rows
    bounds = np.cumsum([len(b) for b in blobs])
    assert {int(b) % 16 for b in bounds} >= {0, 1, 7, 8, 9, 15}
    assert bounds[7] % 4096 == 0 and bounds[7] > 0
    assert bounds[-1] <= 72 << 10
    return blobs


def _write_files(tmp_path, blobs, names=None):
    return [_put(tmp_path / (names[k] if names else f"part-{k:05d}.tfrecord"),
                 b) for k, b in enumerate(blobs)]


def _cpu_reference(raws, schema, record_type):
    """Each file's bytes decoded alone on the CPU engine: (rows of all
    files in order, rows per file)."""
    rows, counts = [], []
    for raw in raws:
        if not raw:
            counts.append(0)
            continue
        batch = cpu_engine.decode_buffer(np.frombuffer(raw, np.uint8), schema,
                                         record_type)
        rows += batch_to_table(batch).to_pylist()
        counts.append(batch.num_rows)
    return rows, counts


def _check_read(paths, raws, schema, record_type, want_schema=None, **kw):
    g = _g()
    batch, row_counts = g.read_files_to_batch(paths, schema, record_type, **kw)
    want_schema = want_schema or schema
    assert batch.schema == want_schema
    want_rows, want_counts = _cpu_reference(raws, want_schema, record_type)
    assert row_counts.tolist() == want_counts
    assert batch.num_rows == len(want_rows)
    assert batch_to_table(g.batch_to_host(batch)).to_pylist() == want_rows


ROUTES = ("pinned", "staged", "staged_4k")


def _take_route(monkeypatch, route):
    if route != "pinned":
        _register_nothing(monkeypatch)
    if route == "staged_4k":
        monkeypatch.setattr(_g(), "_CHUNK", 4096)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("record_type", ["Example", "ByteArray"])
def test_file_boundaries(tmp_path, monkeypatch, record_type, route):
    blobs = _planned_files(record_type)
    paths = _write_files(tmp_path, blobs)
    schema = (EXAMPLE_SCHEMA if record_type == "Example"
              else byte_array_schema())
    _take_route(monkeypatch, route)
    _check_read(paths, blobs, schema, record_type)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("record_type", ["Example", "ByteArray"])
def test_file_boundaries_schema_inferred(tmp_path, monkeypatch, record_type,
                                         route):
    # fused inference: from the first file that has records, which is not
    # file 0
    blobs = _planned_files(record_type)
    assert not blobs[0] and blobs[1]
    paths = _write_files(tmp_path, blobs)
    want_schema = infer_schema_of_paths(paths, record_type, "cpu")
    _take_route(monkeypatch, route)
    _check_read(paths, blobs, None, record_type, want_schema=want_schema)


@pytest.mark.parametrize("route", ["pinned", "staged"])
def test_all_files_empty(tmp_path, monkeypatch, route):
    g = _g()
    paths = _write_files(tmp_path, [b"", b"", b""])
    _take_route(monkeypatch, route)
    batch, row_counts = g.read_files_to_batch(paths, EXAMPLE_SCHEMA, "Example")
    assert batch.num_rows == 0 and batch.schema == EXAMPLE_SCHEMA
    assert row_counts.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="Could not infer schema"):
        g.read_files_to_batch(paths, None, "Example")


def _decoy_files(record_type):
    """Three files; the last record of the middle one holds a fake frame
    header. In the ByteArray file its length leads exactly to the file's
    end, where the next file's first frame starts."""
    if record_type == "ByteArray":
        tail = F.filler(21, 7)
        # a whole fake frame: header, the tail as its payload, and the real
        # frame's CRC word where its own would be
        last = F.filler(30, 8) + F.header(len(tail)) + tail
        mid = _bytes_file(10, 5, 0) + F.frame(last)
        return [_bytes_file(0, 9, 3), mid, _bytes_file(20, 11, 0)]
    ids = range(50, 56)
    bs = [b"z" * (i % 5) for i in ids]
    bs[-1] = b"q" * 9 + F.header(5) + b"y" * 40
    cols = [
        column_from_values(bs, stf.BinaryType(), True, "b"),
        column_from_values([[1.5, float(i)] for i in ids],
                           stf.ArrayType(stf.FloatType()), True, "v"),
        column_from_values(list(ids), stf.LongType(), True, "x"),
    ]
    mid = cpu_engine.encode_batch(RecordBatch(EXAMPLE_SCHEMA, cols, 6),
                                  "Example")
    return [_example_file(0, 9, 3), mid, _example_file(20, 11, 0)]


@pytest.mark.parametrize("record_type", ["Example", "ByteArray"])
def test_decoy_before_a_file_boundary(tmp_path, record_type):
    blobs = _decoy_files(record_type)
    image = b"".join(blobs)
    pos, _ = F.ref_candidates(image, [(0, len(image))])
    frames, _ = F.walk(image)
    decoys = sorted(set(pos.tolist()) - set(frames.tolist()))
    lo, hi = len(blobs[0]), len(blobs[0]) + len(blobs[1])
    assert len(decoys) == 1 and lo < decoys[0] < hi  # the stitch is needed
    if record_type == "ByteArray":
        k = pos.tolist().index(decoys[0])
        assert pos[k + 1] == hi  # and the decoy's own link holds
    paths = _write_files(tmp_path, blobs)
    schema = (EXAMPLE_SCHEMA if record_type == "Example"
              else byte_array_schema())
    _check_read(paths, blobs, schema, record_type)


def test_mixed_codecs_staged(tmp_path, monkeypatch):
    raws = [_example_file(0, 300, 0), _example_file(300, 250, 5), b"",
            _example_file(550, 400, 1), _example_file(950, 120, 0)]
    names = ["part-00000.tfrecord", "part-00001.tfrecord.gz",
             "part-00002.tfrecord", "part-00003.tfrecord.snappy",
             "part-00004.tfrecord"]
    files = [raws[0], P.compress_bytes(raws[1], "gzip"), raws[2],
             P.compress_bytes(raws[3], "snappy"), raws[4]]
    paths = _write_files(tmp_path, files, names)
    _register_nothing(monkeypatch)
    g = _g()
    assert [g.device_source(p).kind for p in paths] == [
        "raw", "gzip", "raw", "snappy", "raw"]
    _check_read(paths, raws, EXAMPLE_SCHEMA, "Example")


# ---------------------------------------------------------------------------
# The staged route with the stream busy
# ---------------------------------------------------------------------------

RACE_SIZES = (70001, 50000, 60007)  # all below _CHUNK: all through half 0
BLOCKER_CAP = 0.5  # seconds


def _random_files(tmp_path, sizes, seed):
    rng = np.random.default_rng(seed)
    blobs = [rng.integers(0, 256, n).astype(np.uint8) for n in sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    paths = [_put(tmp_path / f"r{k}.bin", b.tobytes())
             for k, b in enumerate(blobs)]
    return blobs, list(zip(paths, sizes, offs))


class _Blocker:
    """Work that keeps the current stream busy for a set time: a spin
    kernel where torch's is calibrated, else matmul launches; either way
    timed here, once."""

    def __init__(self):
        import torch
        self.cycles = 2_000_000
        spin = lambda: torch.cuda._sleep(self.cycles)
        spin()
        per = self._time(spin, 2)
        if per >= 2e-4:
            self.spin_rate = self.cycles / per  # cycles per second
            return
        self.spin_rate = None
        a = torch.ones(2048, 2048, device="cuda")
        c = torch.empty_like(a)
        self.mm = lambda: torch.mm(a, a, out=c)
        self.mm()
        self.mm_seconds = self._time(self.mm, 8)

    @staticmethod
    def _time(op, reps):
        import torch
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            op()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3 / reps

    def enqueue(self, seconds):
        """Block the current stream for `seconds`; the event behind it."""
        import torch
        if self.spin_rate:
            torch.cuda._sleep(int(self.spin_rate * seconds))
        else:
            for _ in range(max(1, round(seconds / self.mm_seconds))):
                self.mm()
        ev = torch.cuda.Event()
        ev.record()
        return ev


@pytest.fixture(scope="module")
def blocker(tmp_path_factory):
    """(blocker, seconds): seconds = 20 x one _upload_files of the race's
    three files over an idle stream, registration refused; at most 0.5 s."""
    import torch
    g = _g()
    _, entries = _random_files(tmp_path_factory.mktemp("idle"), RACE_SIZES, 1)
    dst = torch.zeros(sum(RACE_SIZES), dtype=torch.uint8, device="cuda")
    real = _native.file_mmap_pinned
    _native.file_mmap_pinned = lambda path, n, writable: (0, False)
    try:
        g._upload_files(dst, entries)  # the staging buffer's allocation
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g._upload_files(dst, entries)
        torch.cuda.synchronize()
        idle = time.perf_counter() - t0
    finally:
        _native.file_mmap_pinned = real
    return _Blocker(), min(20 * idle, BLOCKER_CAP)


def _upload_behind_blocker(monkeypatch, blocker, entries, total, arm_at=0):
    """_upload_files(entries) with registration refused and the blocker put
    on the stream just before staged chunk `arm_at` is read from its file.
    Returns the image and, per file, whether the blocker had run out when
    the host left that file's staged read."""
    import torch
    g = _g()
    block, seconds = blocker
    _register_nothing(monkeypatch)
    state = {"preads": 0, "event": None}
    left_with_blocker_done = []
    real_pread = _native.pread_parallel
    real_staged = g._read_file_staged

    def pread(fd, ptr, n, pos):
        if state["preads"] == arm_at:
            state["event"] = block.enqueue(seconds)
        state["preads"] += 1
        return real_pread(fd, ptr, n, pos)

    def staged(path, dev):
        out = real_staged(path, dev)
        ev = state["event"]
        left_with_blocker_done.append(ev is None or ev.query())
        return out

    monkeypatch.setattr(_native, "pread_parallel", pread)
    monkeypatch.setattr(g, "_read_file_staged", staged)
    dst = torch.zeros(total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g._upload_files(dst, entries)
    torch.cuda.current_stream().synchronize()
    return dst.cpu().numpy(), left_with_blocker_done


def test_staged_files_behind_a_busy_stream(tmp_path, monkeypatch, blocker):
    """Three small files share half 0 of the staging buffer. The host leaves
    the first file's staged read with its copy still queued behind the
    blocker (asserted: else the blocker is too short to show anything) and
    must not refill the half before that copy has run.

    Where this looks: when the host goes on to the second file, not after
    the whole upload. A staged read that guards the shared half has to wait
    there for the first copy, hence for the blocker, so after the upload
    the blocker has always run out."""
    blobs, entries = _random_files(tmp_path, RACE_SIZES, 2)
    got, left_done = _upload_behind_blocker(
        monkeypatch, blocker, entries, sum(RACE_SIZES))
    assert len(left_done) == 3
    assert not left_done[0], "blocker too short: nothing was queued behind it"
    for k, (b, (_, n, off)) in enumerate(zip(blobs, entries)):
        assert np.array_equal(got[off:off + n], b), f"file {k}"


def test_staged_last_chunk_behind_a_busy_stream(tmp_path, monkeypatch,
                                                blocker):
    """A file of three 4 KiB chunks ends in half 0, where the next file
    starts. The blocker goes on the stream before the first file's last
    chunk (its earlier chunks wait for each other inside the call), so that
    chunk's copy is still queued when the second file wants the half."""
    g = _g()
    monkeypatch.setattr(g, "_CHUNK", 4096)
    sizes = (2 * 4096 + 500, 3000)
    blobs, entries = _random_files(tmp_path, sizes, 3)
    got, left_done = _upload_behind_blocker(
        monkeypatch, blocker, entries, sum(sizes), arm_at=2)
    assert len(left_done) == 2
    assert not left_done[0], "blocker too short: nothing was queued behind it"
    for k, (b, (_, n, off)) in enumerate(zip(blobs, entries)):
        assert np.array_equal(got[off:off + n], b), f"file {k}"


def test_shards_read_staged_behind_a_busy_stream(tmp_path, monkeypatch,
                                                 blocker):
    # the read of docs/ROADMAP.md item 9: 8 freshly written shards, no
    # mapping registers, and the stream still busy when the upload starts
    n = 2000
    rng = np.random.default_rng(4)
    data = {"x": np.arange(n, dtype=np.int64),
            "s": [f"row-{i % 13}" * (i % 5) for i in range(n)],
            "f": rng.random(n).astype(np.float32)}
    out = str(tmp_path / "shards")
    stf.write_tfrecord(data, out, num_shards=8, engine="gpu")
    files = P.list_data_files(out)
    assert len(files) == 8 and all(os.path.getsize(f) for f in files)
    want = stf.read_tfrecord(out, engine="cpu")
    _register_nothing(monkeypatch)
    block, seconds = blocker
    block.enqueue(seconds)
    got = stf.read_tfrecord(out, engine="gpu")
    assert got.schema == want.schema
    key = lambda df: [(r["x"], r["s"], r["f"]) for r in df.collect()]
    assert key(got) == key(want) and len(key(got)) == n
