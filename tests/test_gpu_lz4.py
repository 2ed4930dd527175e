"""GPU tests of the device LZ4 decoder (csrc/hip/lz4.hip) and of the
GPU-engine reads built on it: the cases of tests/test_lz4_codec.py through
the kernel (the CPU tier and csrc/tests/lz4_selftest.cpp ran them through
the same core first), byte-equal to pyarrow's decode, then whole reads
against the CPU engine's. Malformed blocks must come back as error words,
never as a fault."""

import numpy as np
import pytest

import spark_tfrecord_amd as stf
import test_lz4_codec as C
from spark_tfrecord_amd.io import paths as P

pytestmark = pytest.mark.gpu

FILES = {k: (C.one_block_file(c, len(w)), w) for k, (c, w) in C.VALID.items()}
FILES.update(C.container_files())
BAD = {k: (C.one_block_file(c, cap), cause) for k, (c, cap, cause) in C.BAD.items()}


def _gpu_engine():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _write(tmp_path, name, blob):
    p = tmp_path / f"{name}.tfrecord.lz4"
    p.write_bytes(blob)
    return str(p)


def _bytes(dev):
    return dev.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", FILES)
def test_file_on_device(tmp_path, name):
    g = _gpu_engine()
    img, want = FILES[name]
    p = _write(tmp_path, name, img)
    dev = g.read_lz4_file_to_device(p)
    assert dev is not None, g.last_lz4
    assert _bytes(dev) == want
    assert g.last_lz4 == [(p, len(P.lz4_walk(img, name)[0]), -1)]


def test_all_cases_in_one_launch(tmp_path):
    """Clean and malformed files as one group: each malformed file gets its
    error word, the clean ones decode beside them."""
    import torch

    g = _gpu_engine()
    named = [(k, img, len(w)) for k, (img, w) in FILES.items() if w] + \
            [(k, img, C._N) for k, (img, _) in BAD.items()]
    items, base = [], 0
    for name, img, n in named:
        p = _write(tmp_path, name, img)
        meta = g.lz4_device_meta(p)
        assert meta is not None and meta[1] == n, name
        items.append((p, meta, base))
        base += n
    data = torch.full((base,), 0xEE, dtype=torch.uint8, device="cuda")
    ok = g._device_unlz4_group(data, items, "cuda")
    flat = _bytes(data)
    for (name, _, n), it, good, last in zip(named, items, ok, g.last_lz4):
        if name in BAD:
            assert not good and last[2] == (1 << 8) | BAD[name][1], name
        else:
            assert good and last[2] == -1, name
            assert flat[it[2]:it[2] + n] == FILES[name][1], name


@pytest.mark.parametrize("name", BAD)
def test_malformed_file_raises(tmp_path, name):
    d = tmp_path / "ds"
    d.mkdir()
    _write(d, name, BAD[name][0])
    with pytest.raises(ValueError, match="lz4"):
        stf.read_tfrecord(str(d), engine="gpu")


def test_more_blocks_than_resident_waves(tmp_path):
    """One file of (launch's wave cap + 1000) blocks of 64 raw bytes: the
    later blocks are reached only through the grid-stride loop."""
    g = _gpu_engine()
    n = g._lz4_max_waves("cuda") + 1000
    raw = np.random.default_rng(9).integers(0, 256, (n, 64)).astype(np.uint8)
    img = b"".join(C.one_block_file(C.seq(raw[k].tobytes()), 64) for k in range(n))
    p = _write(tmp_path, "many", img)
    dev = g.read_lz4_file_to_device(p)
    assert dev is not None, g.last_lz4
    assert g.last_lz4 == [(p, n, -1)]
    assert _bytes(dev) == raw.tobytes()


@pytest.mark.parametrize("where", ["device", "host"])
def test_read_equals_cpu_engine(tmp_path, monkeypatch, where):
    monkeypatch.setenv("TFREC_LZ4", where)
    g = _gpu_engine()
    rows = {"x": np.arange(6000, dtype=np.int64),
            "s": [f"row-{i % 13}" for i in range(6000)]}
    d = str(tmp_path / "out")
    stf.write_tfrecord(rows, d, codec="lz4", engine="gpu", num_shards=3)
    assert all(f.endswith(".lz4") for f in P.list_data_files(d))
    del g.last_lz4[:]
    got, want = (sorted((r["x"], r["s"]) for r in stf.read_tfrecord(d, engine=e).collect())
                 for e in ("gpu", "cpu"))
    assert got == want == sorted(zip(rows["x"].tolist(), rows["s"]))
    assert (len(g.last_lz4) == 3 and all(e[2] == -1 for e in g.last_lz4)) == (where == "device")
