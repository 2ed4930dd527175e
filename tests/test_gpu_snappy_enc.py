"""GPU tests of the device Snappy compressor (csrc/hip/snappy_enc.hip) and
of the snappy_engine="device" write path built on it.

The device image must equal, byte for byte, the image assembled on the host
from the host build of the same core (tests/test_snappy_enc_core.py checks
that one against the library); it must also read back through the library,
through the project's CPU reader and through the device decoder."""

import os

import numpy as np
import pyarrow as pa
import pytest

import snappy_enc_cases as C
import spark_tfrecord_amd as stf
from spark_tfrecord_amd.io import paths as P

pytestmark = pytest.mark.gpu

CASES = C.cases()


def _gpu_engine():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _device_image(data: bytes, block=None) -> bytes:
    import torch
    g = _gpu_engine()
    img = torch.frombuffer(bytearray(data) or bytearray(1),
                           dtype=torch.uint8)[:len(data)].cuda()
    return g.snappy_image_device(img, block).cpu().numpy().tobytes()


def _check_image(tmp_path, name, data, block):
    g = _gpu_engine()
    dev = _device_image(data, block)
    assert dev == C.host_snappy_image(data, block), "device != host core"
    assert _device_image(data, block) == dev, "two device runs differ"
    assert P.snappy_decompress(dev, name) == data
    p = str(tmp_path / f"{name}.tfrecord.snappy")
    with open(p, "wb") as f:
        f.write(dev)
    back = g.read_snappy_file_to_device(p)
    assert back is not None, g.last_snappy
    assert back.cpu().numpy().tobytes() == data


@pytest.mark.parametrize("name,data,block", CASES, ids=[c[0] for c in CASES])
def test_device_image(tmp_path, name, data, block):
    _check_image(tmp_path, name, data, block)


def test_default_block_size():
    data = [c for c in CASES if c[0] == "example_200_rows"][0][1] * 4
    assert len(data) > 2 * P.snappy_block_size()
    assert _device_image(data) == C.host_snappy_image(
        data, P.snappy_block_size())


def test_more_blocks_than_resident_waves(tmp_path):
    # the later blocks are reached only through the grid-stride loop
    g = _gpu_engine()
    nblk = g._snap_max_waves("cuda") + 1000
    text = C._rand(11, nblk * 64 - 5, 97, 123)
    _check_image(tmp_path, "stride", text, 64)


def test_empty_image_is_zero_bytes():
    import torch
    g = _gpu_engine()
    out = g.snappy_image_device(torch.empty(0, dtype=torch.uint8,
                                            device="cuda"))
    assert out.numel() == 0 and out.dtype == torch.uint8 and out.is_cuda


def test_block_above_the_cap_raises():
    import torch
    g = _gpu_engine()
    img = torch.zeros(100, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="block size"):
        g.snappy_image_device(img, g.SNAPPY_MAX_CHUNK_RAW + 1)
    assert g.snappy_image_device(img, g.SNAPPY_MAX_CHUNK_RAW).numel() > 0
    with pytest.raises(ValueError):
        g.snappy_image_device(img, 0)


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


@pytest.fixture
def device_calls(monkeypatch):
    """Counts the compressions that ran on the device."""
    g = _gpu_engine()
    calls = []
    real = g.snappy_image_device
    monkeypatch.setattr(
        g, "snappy_image_device",
        lambda img, block=None: calls.append(1) or real(img, block))
    return calls


def _check_dataset(out, table, n_files, **read_kw):
    files = P.list_data_files(out)
    assert len(files) == n_files
    for f in files:
        assert f.endswith(".snappy")
        with open(f, "rb") as fh:
            blob = fh.read()
        chunks, total = P.snappy_walk(blob, f)
        assert total > 0 and len(chunks) == -(-total // P.snappy_block_size())
    want = table.sort_by("id").to_pylist()
    for eng in ("cpu", "gpu"):
        got = stf.read_tfrecord(out, engine=eng, **read_kw).sort("id").collect()
        assert len(got) == len(want), eng
        for a, b in zip(got, want):
            assert a["id"] == b["id"] and a["name"] == b["name"], eng
            assert a["part"] == b["part"], eng
            assert a["score"] == pytest.approx(b["score"], rel=0, abs=0), eng


def test_write_single_shard(tmp_sandbox, example_table, device_calls):
    out = str(tmp_sandbox / "one")
    stf.write_tfrecord(example_table, out, engine="gpu", codec="snappy",
                       snappy_engine="device")
    assert device_calls == [1]
    _check_dataset(out, example_table, 1)


def test_write_three_shards(tmp_sandbox, example_table, device_calls):
    out = str(tmp_sandbox / "three")
    stf.write_tfrecord(example_table, out, engine="gpu", codec="snappy",
                       snappy_engine="device", num_shards=3)
    assert device_calls == [1, 1, 1]
    _check_dataset(out, example_table, 3)


def test_write_three_shards_pooled(tmp_sandbox, example_table, device_calls):
    # >= 32768 rows takes the thread-pool shard path
    big = pa.concat_tables([example_table, example_table.set_column(
        0, "id", pa.array(np.arange(N, 2 * N, dtype=np.int64)))])
    out = str(tmp_sandbox / "pooled")
    stf.write_tfrecord(big, out, engine="gpu", codec="snappy",
                       snappy_engine="device", num_shards=3)
    assert device_calls == [1, 1, 1]
    _check_dataset(out, big, 3)


def test_write_partition_by(tmp_sandbox, example_table, device_calls):
    out = str(tmp_sandbox / "parts")
    stf.write_tfrecord(example_table, out, engine="gpu", codec="snappy",
                       snappy_engine="device", partition_by=["part"])
    assert device_calls == [1, 1, 1]
    assert sorted(d for d in os.listdir(out) if d.startswith("part=")) == \
        ["part=0", "part=1", "part=2"]
    _check_dataset(out, example_table, 3)


def test_device_ignored_without_snappy(tmp_sandbox, device_calls):
    data = {"x": np.arange(100, dtype=np.int64)}
    for codec in (None, "deflate", "gzip"):
        out = str(tmp_sandbox / f"c{codec}")
        stf.write_tfrecord(data, out, engine="gpu", codec=codec,
                           snappy_engine="device")
        got = stf.read_tfrecord(out, engine="cpu").sort("x").collect()
        assert [r["x"] for r in got] == list(range(100))
    assert device_calls == []


def test_large_block_goes_to_the_host(tmp_sandbox, monkeypatch, device_calls):
    monkeypatch.setattr(P, "_SNAPPY_BLOCK", (1 << 20) + 1)
    data = {"x": np.arange(1000, dtype=np.int64)}
    out = str(tmp_sandbox / "big_block")
    stf.write_tfrecord(data, out, engine="gpu", codec="snappy",
                       snappy_engine="device")
    assert device_calls == []
    got = stf.read_tfrecord(out, engine="cpu").sort("x").collect()
    assert [r["x"] for r in got] == list(range(1000))


def test_option_reaches_writer(tmp_sandbox, example_table, monkeypatch,
                               device_calls):
    session = stf.TFRecordSession()
    small = example_table.slice(0, 500)
    df = session.createDataFrame(small)
    out = str(tmp_sandbox / "opt")
    df.write.format("tfrecord").option("codec", "snappy") \
        .option("engine", "gpu").option("snappyEngine", "device").save(out)
    assert device_calls == [1]
    _check_dataset(out, small, 1)
    # the default stays on the host, and the environment moves it
    out2 = str(tmp_sandbox / "opt2")
    df.write.format("tfrecord").option("codec", "snappy") \
        .option("engine", "gpu").save(out2)
    assert device_calls == [1]
    monkeypatch.setenv("TFREC_SNAPPY_ENGINE", "device")
    out3 = str(tmp_sandbox / "opt3")
    df.write.format("tfrecord").option("codec", "snappy") \
        .option("engine", "gpu").save(out3)
    assert device_calls == [1, 1]
    _check_dataset(out3, small, 1)
