"""GPU tests of the device DEFLATE compressor (csrc/hip/deflate.hip) and of
the gzip_engine="device" write path built on it.

The device image must equal, byte for byte, the image assembled on the host
from the host build of the same core (tests/test_deflate_core.py checks that
one against zlib); it must also read back through gzip, through the
project's CPU reader and through the device inflater."""

import gzip
import os

import numpy as np
import pyarrow as pa
import pytest

import deflate_cases as C
import spark_tfrecord_amd as stf
from spark_tfrecord_amd.io import paths as P

pytestmark = pytest.mark.gpu

CASES = C.cases()


def _gpu_engine():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _device_image(data: bytes, seg=None) -> bytes:
    import torch
    g = _gpu_engine()
    img = torch.frombuffer(bytearray(data) or bytearray(1),
                           dtype=torch.uint8)[:len(data)].cuda()
    return g.gzip_image_device(img, seg).cpu().numpy().tobytes()


def _check_image(tmp_path, name, data, seg):
    g = _gpu_engine()
    dev = _device_image(data, seg)
    assert dev == C.host_gzip_image(data, seg), "device != host core"
    assert gzip.decompress(dev) == data
    assert _device_image(data, seg) == dev, "two device runs differ"
    p = str(tmp_path / f"{name}.tfrecord.gz")
    with open(p, "wb") as f:
        f.write(dev)
    back = g.read_gzip_file_to_device(p)
    assert back is not None, "device inflater rejected the image"
    assert back.cpu().numpy().tobytes() == data


@pytest.mark.parametrize("name,data,seg", CASES, ids=[c[0] for c in CASES])
def test_device_image(tmp_path, name, data, seg):
    _check_image(tmp_path, name, data, seg)


def test_default_segment_size():
    data = [c for c in CASES if c[0] == "alpha25"][0][1] * 2 + b"tail"
    assert _device_image(data) == C.host_gzip_image(
        data, P._gz_segment_size(len(data)))


def test_many_segments_one_launch(tmp_path):
    # every 32 KiB input in one image: several blocks of waves in one launch
    full = b"".join(d for _, d, s in CASES
                    if s == C.SEG and len(d) == C.SEG) + b"tail"
    assert len(full) == 5 * C.SEG + 4
    _check_image(tmp_path, "multi", full, C.SEG)
    # more segments than resident waves: the grid-stride loop, its reused
    # token workspace, and the threaded CRC fold of the assemble kernel
    g = _gpu_engine()
    nseg = g._deflate_max_waves("cuda") + 1000
    text = C._rand(11, nseg * 64 - 5, 97, 122)
    _check_image(tmp_path, "stride", text, 64)


def test_too_many_segments_raises():
    import torch
    g = _gpu_engine()
    img = torch.zeros(P._GZ_MAX_SEGS * 16 + 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        g.gzip_image_device(img, 16)
    assert len(g.gzip_image_device(img[:-1], 16)) > 0  # exactly the cap fits


# ---- end to end ------------------------------------------------------------

N = 20_000


@pytest.fixture(scope="module")
def example_table():
    rng = np.random.default_rng(0)
    return pa.table({
        "id": np.arange(N, dtype=np.int64),
        "part": (np.arange(N) % 3).astype(np.int64),
        "score": rng.random(N).astype(np.float32),
        "name": [f"user-{i % 997}" for i in range(N)],
    })


def _check_dataset(out, table, n_files, **read_kw):
    files = P.list_data_files(out)
    assert len(files) == n_files
    for f in files:
        assert f.endswith(".gz")
        assert P.parse_gz_segments_file(f) is not None
        assert len(gzip.decompress(open(f, "rb").read())) > 0
    want = table.sort_by("id").to_pylist()
    for eng in ("cpu", "gpu"):
        got = stf.read_tfrecord(out, engine=eng, **read_kw).sort("id").collect()
        assert len(got) == len(want), eng
        for a, b in zip(got, want):
            assert a["id"] == b["id"] and a["name"] == b["name"], eng
            assert a["part"] == b["part"], eng
            assert a["score"] == pytest.approx(b["score"], rel=0, abs=0), eng


def test_write_single_shard(tmp_sandbox, example_table):
    out = str(tmp_sandbox / "one")
    stf.write_tfrecord(example_table, out, engine="gpu", codec="gzip",
                       gzip_engine="device")
    _check_dataset(out, example_table, 1)


def test_write_three_shards(tmp_sandbox, example_table):
    out = str(tmp_sandbox / "three")
    stf.write_tfrecord(example_table, out, engine="gpu", codec="gzip",
                       gzip_engine="device", num_shards=3)
    _check_dataset(out, example_table, 3)


def test_write_three_shards_pooled(tmp_sandbox, example_table):
    # >= 32768 rows takes the thread-pool shard path
    big = pa.concat_tables([example_table, example_table.set_column(
        0, "id", pa.array(np.arange(N, 2 * N, dtype=np.int64)))])
    out = str(tmp_sandbox / "pooled")
    stf.write_tfrecord(big, out, engine="gpu", codec="gzip",
                       gzip_engine="device", num_shards=3)
    _check_dataset(out, big, 3)


def test_write_partition_by(tmp_sandbox, example_table):
    out = str(tmp_sandbox / "parts")
    stf.write_tfrecord(example_table, out, engine="gpu", codec="gzip",
                       gzip_engine="device", partition_by=["part"])
    assert sorted(d for d in os.listdir(out) if d.startswith("part=")) == \
        ["part=0", "part=1", "part=2"]
    _check_dataset(out, example_table, 3)


def test_write_byte_array(tmp_sandbox):
    rng = np.random.default_rng(5)
    payloads = [rng.bytes(200) for _ in range(N)]
    t = pa.table({"byteArray": pa.array(payloads, type=pa.large_binary())})
    out = str(tmp_sandbox / "ba")
    stf.write_tfrecord(t, out, record_type="ByteArray", engine="gpu",
                       codec="gzip", gzip_engine="device")
    files = P.list_data_files(out)
    assert len(files) == 1 and P.parse_gz_segments_file(files[0]) is not None
    for eng in ("cpu", "gpu"):
        df = stf.read_tfrecord(out, record_type="ByteArray", engine=eng)
        assert [r["byteArray"] for r in df.collect()] == payloads, eng


def test_device_needs_gpu_engine(tmp_sandbox):
    with pytest.raises(ValueError):
        stf.write_tfrecord({"x": np.arange(10, dtype=np.int64)},
                           str(tmp_sandbox / "cpu"), engine="cpu",
                           codec="gzip", gzip_engine="device")
    with pytest.raises(ValueError):
        stf.write_tfrecord({"x": np.arange(10, dtype=np.int64)},
                           str(tmp_sandbox / "bad"), engine="gpu",
                           codec="gzip", gzip_engine="fpga")


def test_device_ignored_without_gzip(tmp_sandbox):
    data = {"x": np.arange(100, dtype=np.int64)}
    for codec in (None, "deflate"):
        out = str(tmp_sandbox / f"c{codec}")
        stf.write_tfrecord(data, out, engine="gpu", codec=codec,
                           gzip_engine="device")
        got = stf.read_tfrecord(out, engine="cpu").sort("x").collect()
        assert [r["x"] for r in got] == list(range(100))


def test_option_reaches_writer(tmp_sandbox, example_table, monkeypatch):
    g = _gpu_engine()
    calls = []
    real = g.gzip_image_device
    monkeypatch.setattr(g, "gzip_image_device",
                        lambda img, seg=None: calls.append(1) or real(img, seg))
    session = stf.TFRecordSession()
    df = session.createDataFrame(example_table.slice(0, 500))
    out = str(tmp_sandbox / "opt")
    df.write.format("tfrecord").option("codec", "gzip") \
        .option("engine", "gpu").option("gzipEngine", "device").save(out)
    assert calls == [1]
    _check_dataset(out, example_table.slice(0, 500), 1)
    # the default stays on the host, and the environment moves it
    out2 = str(tmp_sandbox / "opt2")
    df.write.format("tfrecord").option("codec", "gzip") \
        .option("engine", "gpu").save(out2)
    assert calls == [1]
    monkeypatch.setenv("TFREC_GZ_ENGINE", "device")
    out3 = str(tmp_sandbox / "opt3")
    df.write.format("tfrecord").option("codec", "gzip") \
        .option("engine", "gpu").save(out3)
    assert calls == [1, 1]
