"""GPU tests of the device Snappy decoder (csrc/hip/snappy.hip) and of the
GPU-engine read paths built on it: the cases of tests/snappy_cases.py
through the kernel (the CPU tier ran them through the same core first),
then whole reads against the CPU engine's read of the same files. Malformed
chunks must come back as error words, never as a fault."""

import os
import struct

import numpy as np
import pytest

import snappy_cases as C
import spark_tfrecord_amd as stf
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P

pytestmark = pytest.mark.gpu

CHUNKS = C.valid_chunks()
FILES = C.valid_files()
BAD_CHUNKS = C.malformed_chunks()
BAD_FILES = C.malformed_files()


def _gpu_engine():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _write(tmp_path, name, blob):
    p = str(tmp_path / f"{name}.tfrecord.snappy")
    with open(p, "wb") as f:
        f.write(blob)
    return p


def _bytes(dev):
    return dev.cpu().numpy().tobytes()


@pytest.mark.parametrize("name,comp,want", CHUNKS, ids=[c[0] for c in CHUNKS])
def test_chunk_on_device(tmp_path, name, comp, want):
    g = _gpu_engine()
    p = _write(tmp_path, name, C.one_chunk_file(comp, want))
    dev = g.read_snappy_file_to_device(p)
    assert dev is not None, g.last_snappy
    got = _bytes(dev)
    assert got == want
    assert got == _native.host_unsnap_chunk(comp, len(want))
    assert g.last_snappy == [(p, 1 if want else 0, -1)]


@pytest.mark.parametrize("name,img,want", FILES, ids=[f[0] for f in FILES])
def test_file_on_device(tmp_path, name, img, want):
    g = _gpu_engine()
    p = _write(tmp_path, name, img)
    dev = g.read_snappy_file_to_device(p)
    assert dev is not None, g.last_snappy
    assert _bytes(dev) == want
    (path, nchunk, err), = g.last_snappy
    assert err == -1 and nchunk == len(P.snappy_walk(img, name)[0])


def _group(g, tmp_path, named):
    """Decode [(name, image, want)] as the files of one group, in one
    launch; returns (ok flags, [each file's bytes])."""
    import torch

    items = []
    base = 0
    for name, img, want in named:
        p = _write(tmp_path, name, img)
        meta = g.snappy_device_meta(p)
        assert meta is not None and meta[1] == len(want), name
        items.append((p, meta, base))
        base += len(want)
    data = torch.full((base,), 0xEE, dtype=torch.uint8, device="cuda")
    ok = g._device_unsnap_group(data, items, "cuda")
    flat = _bytes(data)
    return ok, [flat[it[2]:it[2] + it[1][1]] for it in items]


def test_all_cases_in_one_launch(tmp_path):
    g = _gpu_engine()
    named = [(f"c_{n}", C.one_chunk_file(c, w), w) for n, c, w in CHUNKS] + \
            [(f"f_{n}", img, w) for n, img, w in FILES]
    ok, got = _group(g, tmp_path, named)
    assert ok == [True] * len(named)
    for (name, _, want), have in zip(named, got):
        assert have == want, name
    assert [e[2] for e in g.last_snappy] == [-1] * len(named)
    assert sum(e[1] for e in g.last_snappy) > len(named)  # multi-chunk files


def test_more_chunks_than_resident_waves(tmp_path):
    """One file of (launch's wave cap + 1000) chunks of 64 raw bytes: the
    later chunks are reached only through the grid-stride loop."""
    g = _gpu_engine()
    n = g._snappy_max_waves("cuda") + 1000
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, (n, 64)).astype(np.uint8)
    pre = C.varint(64) + bytes([0xF0, 63])  # 64-byte literal, 1-byte form
    head = struct.pack(">II", 64, len(pre) + 64)
    img = b"".join(head + pre + raw[k].tobytes() for k in range(n))
    p = _write(tmp_path, "many", img)
    dev = g.read_snappy_file_to_device(p)
    assert dev is not None, g.last_snappy
    assert g.last_snappy == [(p, n, -1)]
    assert _bytes(dev) == raw.tobytes()


def _frames(tmp_path, tag, lo, hi):
    """Raw TFRecord frames of rows lo..hi, written by the project itself."""
    d = str(tmp_path / f"src_{tag}")
    stf.write_tfrecord(
        {"x": np.arange(lo, hi, dtype=np.int64),
         "s": [f"row-{i % 13}" for i in range(lo, hi)]},
        d, engine="cpu")
    (f,) = P.list_data_files(d)
    with open(f, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("name,comp,expect_len,cause", BAD_CHUNKS,
                         ids=[c[0] for c in BAD_CHUNKS])
def test_malformed_chunk_is_refused(tmp_path, name, comp, expect_len, cause):
    import torch

    g = _gpu_engine()
    out = tmp_path / "dir"
    out.mkdir()
    raws = [_frames(tmp_path, "a", 0, 300), _frames(tmp_path, "b", 300, 900)]
    good = [_write(out, f"part-0000{k}", P.compress_bytes(r, "snappy"))
            for k, r in zip((0, 2), raws)]
    bad = _write(out, "part-00001",
                 struct.pack(">II", expect_len, len(comp)) + comp)
    # the extents as the 8 header bytes give them: the kernel is the one
    # to look at the chunk (the read path's header walk also reads the
    # preamble, and refuses the two preamble cases before any launch)
    bad_meta = (np.array([[8, len(comp), 0, expect_len]], np.int64),
                expect_len)
    if cause in (C.SN_PREAMBLE_LONG, C.SN_PREAMBLE_MISMATCH):
        assert g.snappy_device_meta(bad) is None
    else:
        walked = g.snappy_device_meta(bad)
        assert walked is not None and walked[1] == expect_len
        assert np.array_equal(walked[0], bad_meta[0])
    metas = [g.snappy_device_meta(p) for p in good]
    items = [(good[0], metas[0], 0),
             (bad, bad_meta, len(raws[0])),
             (good[1], metas[1], len(raws[0]) + expect_len)]
    total = len(raws[0]) + expect_len + len(raws[1])
    data = torch.zeros(total, dtype=torch.uint8, device="cuda")
    ok = g._device_unsnap_group(data, items, "cuda")
    assert ok == [True, False, True]
    assert [e[2] for e in g.last_snappy] == [-1, (1 << 8) | cause, -1]
    flat = _bytes(data)
    assert flat[:len(raws[0])] == raws[0]
    assert flat[len(raws[0]) + expect_len:] == raws[1]
    # single-file entry point: None, the caller goes to the host
    if g.snappy_device_meta(bad) is not None:
        assert g.read_snappy_file_to_device(bad) is None
        assert g.last_snappy == [(bad, 1, (1 << 8) | cause)]
    # the whole read: the device refuses the file, the host names it
    with pytest.raises(ValueError, match="part-00001"):
        stf.read_tfrecord(str(out), engine="gpu")
    rep = stf.validate_tfrecord(str(out), engine="gpu")
    assert [f.ok for f in rep.files] == [True, False, True]


@pytest.mark.parametrize("name,img", BAD_FILES, ids=[f[0] for f in BAD_FILES])
def test_failed_header_walk_never_reaches_the_kernel(tmp_path, monkeypatch,
                                                     name, img):
    g = _gpu_engine()
    out = tmp_path / "dir"
    out.mkdir()
    p = _write(out, "part-00000", img)
    calls = []
    real = g._device_unsnap_group
    monkeypatch.setattr(g, "_device_unsnap_group",
                        lambda *a: calls.append(a) or real(*a))
    assert g.snappy_device_meta(p) is None
    assert g.read_snappy_file_to_device(p) is None
    with pytest.raises(ValueError, match="part-00000"):
        stf.read_tfrecord(str(out), engine="gpu")
    with pytest.raises(ValueError, match="part-00000"):
        stf.count_tfrecord(str(out), engine="gpu")
    assert calls == []


def test_chunk_above_the_cap_goes_to_the_host(tmp_path, monkeypatch):
    g = _gpu_engine()
    raw = _frames(tmp_path, "a", 0, 2000)
    out = tmp_path / "dir"
    out.mkdir()
    p = _write(out, "part-00000", P.compress_bytes(raw, "snappy"))
    monkeypatch.setattr(g, "SNAPPY_MAX_CHUNK_RAW", 1000)
    assert g.snappy_device_meta(p) is None
    del g.last_snappy[:]
    assert stf.read_tfrecord(str(out), engine="gpu").count() == 2000
    assert g.last_snappy == []


# ---------------------------------------------------------------------------
# end to end: 20,000 rows of the flagship Example schema
# ---------------------------------------------------------------------------

ROWS = 20_000


@pytest.fixture(scope="module")
def flagship(tmp_path_factory):
    """(directory of two snappy shards, the CPU engine's read of it, the
    source table): written and read once for every test below."""
    from bench import make_batch
    from spark_tfrecord_amd.arrow_interop import batch_to_table

    batch = make_batch(ROWS, seed=11)
    table = batch_to_table(batch)
    out = str(tmp_path_factory.mktemp("snappy_e2e") / "data")
    stf.write_tfrecord(table, out, schema=batch.schema, codec="snappy",
                       engine="cpu", num_shards=2)
    files = P.list_data_files(out)
    assert len(files) == 2 and all(f.endswith(".snappy") for f in files)
    cpu = stf.read_tfrecord(out, schema=batch.schema, engine="cpu")
    assert cpu.count() == ROWS
    return out, cpu, table, batch.schema


def _same_columns(a, b):
    ta, tb = a.to_arrow_table(), b.to_arrow_table()
    assert ta.column_names == tb.column_names
    assert ta.num_rows == tb.num_rows
    for c in ta.column_names:
        assert ta.column(c).equals(tb.column(c)), c


def test_read_matches_cpu_engine(flagship):
    g = _gpu_engine()
    out, cpu, _, schema = flagship
    del g.last_snappy[:]
    gpu = stf.read_tfrecord(out, schema=schema, engine="gpu")
    _same_columns(gpu, cpu)
    files = P.list_data_files(out)
    assert [e[0] for e in g.last_snappy] == files  # one group, one launch
    assert all(e[1] > 10 and e[2] == -1 for e in g.last_snappy)


def test_read_with_host_knob(flagship, monkeypatch):
    g = _gpu_engine()
    out, cpu, _, schema = flagship
    monkeypatch.setenv("TFREC_SNAPPY", "host")
    del g.last_snappy[:]
    _same_columns(stf.read_tfrecord(out, schema=schema, engine="gpu"), cpu)
    assert g.last_snappy == []
    monkeypatch.setenv("TFREC_SNAPPY", "neither")
    with pytest.raises(ValueError, match="TFREC_SNAPPY"):
        stf.read_tfrecord(out, schema=schema, engine="gpu")


def test_schema_less_read_fuses_inference(flagship, monkeypatch):
    g = _gpu_engine()
    out, cpu, _, _ = flagship
    seen = []
    real = g.read_files_to_batch
    monkeypatch.setattr(
        g, "read_files_to_batch",
        lambda paths, schema, *a, **k: seen.append(schema) or
        real(paths, schema, *a, **k))
    del g.last_snappy[:]
    gpu = stf.read_tfrecord(out, engine="gpu")
    assert seen == [None]  # inferred inside the one group pipeline
    assert len(g.last_snappy) == 2
    want = stf.read_tfrecord(out, engine="cpu")
    assert gpu.schema == want.schema
    _same_columns(gpu, want)


def test_column_projection(flagship):
    out, cpu, _, schema = flagship
    gpu = stf.read_tfrecord(out, schema=schema, engine="gpu",
                            columns=["id", "tokens"])
    assert gpu.columns == ["id", "tokens"]
    _same_columns(gpu, cpu.select("id", "tokens"))


def test_count_validate_infer(flagship):
    from spark_tfrecord_amd.io.reader import infer_schema_of_paths

    g = _gpu_engine()
    out, cpu, _, _ = flagship
    files = P.list_data_files(out)
    del g.last_snappy[:]
    assert stf.count_tfrecord(out, engine="gpu") == ROWS
    assert g.last_snappy and g.last_snappy[0][2] == -1
    del g.last_snappy[:]
    rep = stf.validate_tfrecord(out, engine="gpu")
    assert rep.ok and rep.records == ROWS and len(rep.files) == 2
    assert g.last_snappy and g.last_snappy[0][2] == -1
    del g.last_snappy[:]
    assert infer_schema_of_paths(files, "Example", "gpu") == \
        infer_schema_of_paths(files, "Example", "cpu")
    assert g.last_snappy and g.last_snappy[0][2] == -1


def test_dataset_over_two_shards(flagship, monkeypatch):
    from spark_tfrecord_amd.torch_data import TFRecordIterableDataset

    g = _gpu_engine()
    out, _, table, schema = flagship

    def values():
        ds = TFRecordIterableDataset(out, schema=schema, engine="gpu",
                                     prefetch=0)
        got = {}
        for item in ds:
            for k, v in item.items():
                got.setdefault(k, []).append(np.atleast_1d(v.cpu().numpy()))
        return {k: np.concatenate(v) for k, v in got.items()}

    del g.last_snappy[:]
    dev = values()
    assert g.last_snappy and g.last_snappy[0][2] == -1  # the second shard
    monkeypatch.setenv("TFREC_SNAPPY", "host")
    del g.last_snappy[:]
    host = values()
    assert g.last_snappy == []
    assert host.keys() == dev.keys()
    for k in host:
        assert np.array_equal(host[k], dev[k]), k
    assert np.array_equal(dev["id"], table.column("id").to_numpy())
    assert np.array_equal(
        dev["ints"], table.column("ints").combine_chunks().flatten().to_numpy())


def test_mixed_directory_is_one_group(tmp_path, monkeypatch):
    g = _gpu_engine()
    out = tmp_path / "mix"
    out.mkdir()
    raws = [_frames(tmp_path, "a", 0, 3000), _frames(tmp_path, "b", 3000, 5000),
            _frames(tmp_path, "c", 5000, 9500)]
    with open(out / "part-00000.tfrecord", "wb") as f:
        f.write(raws[0])
    with open(out / "part-00001.tfrecord.gz", "wb") as f:
        f.write(P.compress_bytes(raws[1], "gzip"))
    with open(out / "part-00002.tfrecord.snappy", "wb") as f:
        f.write(P.compress_bytes(raws[2], "snappy"))
    calls = []
    real = g.read_files_to_batch

    def spy(paths, *a, **k):
        batch, row_counts = real(paths, *a, **k)
        calls.append(([os.path.basename(p) for p in paths],
                      list(map(int, row_counts))))
        return batch, row_counts

    monkeypatch.setattr(g, "read_files_to_batch", spy)
    df = stf.read_tfrecord(str(out), engine="gpu")
    assert calls == [(["part-00000.tfrecord", "part-00001.tfrecord.gz",
                       "part-00002.tfrecord.snappy"], [3000, 2000, 4500])]
    assert [r["x"] for r in df.collect()] == list(range(9500))
    assert g.last_snappy[0][2] == -1


def test_gpu_engine_write_reads_back(tmp_path):
    """The GPU engine's writer takes the codec with no code of its own:
    encode on the device, the container on the host."""
    g = _gpu_engine()
    out = str(tmp_path / "w")
    data = {"x": np.arange(5000, dtype=np.int64),
            "s": [f"row-{i % 13}" for i in range(5000)]}
    stf.write_tfrecord(data, out, codec="snappy", engine="gpu")
    (f,) = P.list_data_files(out)
    assert f.endswith(".tfrecord.snappy")
    del g.last_snappy[:]
    rows = stf.read_tfrecord(out, engine="gpu").collect()
    assert [r["x"] for r in rows] == list(range(5000))
    assert g.last_snappy == [(f, len(P.snappy_walk(open(f, "rb").read(),
                                                   f)[0]), -1)]
