"""GPU tests of the speculative foreign-gzip inflater
(csrc/hip/inflate_foreign.hip) and of the foreign_gzip="device" read path
built on it: the cases of tests/foreign_gz_cases.py through the kernels,
then whole reads against the foreign_gzip="host" read of the same files.
Damaged files must come back as error words (None here), never as a fault.
"""

import os

import numpy as np
import pytest

import foreign_gz_cases as C
import spark_tfrecord_amd as stf
from spark_tfrecord_amd.io import paths as P

pytestmark = pytest.mark.gpu

MAIN = C.main_cases()
VARIANTS = C.variant_cases()
REJECTED = C.rejected_cases()
ACCEPTED = [(n, gz, d, s, cond) for n, gz, d, s, cond in MAIN] + \
           [(n, gz, d, s, None) for n, gz, d, s in VARIANTS]


def _gpu_engine():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _write(tmp_path, name, blob):
    p = str(tmp_path / f"{name}.tfrecord.gz")
    with open(p, "wb") as f:
        f.write(blob)
    return p


@pytest.mark.parametrize("name,gz,data,stride,cond", ACCEPTED,
                         ids=[c[0] for c in ACCEPTED])
def test_device_inflate(tmp_path, name, gz, data, stride, cond):
    g = _gpu_engine()
    p = _write(tmp_path, name, gz)
    dev = g.read_foreign_gzip_file_to_device(p, stride)
    assert dev is not None, g.last_foreign
    assert dev.cpu().numpy().tobytes() == data
    (_, live, markers, err), = g.last_foreign
    assert err == -1
    if cond is not None:
        kind, n = cond
        assert (live >= n) if kind == "min" else (live == n), live
    if name == "dyn_small_blocks":
        assert markers > 0
    again = g.read_foreign_gzip_file_to_device(p, stride)
    assert again is not None and bool((again == dev).all())
    assert g.last_foreign[0][1:] == (live, markers, err)
    assert g.read_gzip_file_to_device(p) is None  # still no segment table


@pytest.mark.parametrize("stride", [1024, 32768, 1 << 20])
def test_other_strides(tmp_path, stride):
    g = _gpu_engine()
    name, gz, data, _, _ = MAIN[0]
    dev = g.read_foreign_gzip_file_to_device(_write(tmp_path, name, gz),
                                             stride)
    assert dev is not None and dev.cpu().numpy().tobytes() == data


@pytest.mark.parametrize("name,gz,host", REJECTED,
                         ids=[c[0] for c in REJECTED])
def test_device_refuses(tmp_path, name, gz, host):
    g = _gpu_engine()
    p = _write(tmp_path, name, gz)
    assert g.read_foreign_gzip_file_to_device(p, 2048) is None
    assert g.read_foreign_gzip_file_to_device(p) is None


def test_empty_payload_is_ineligible(tmp_path):
    g = _gpu_engine()
    p = _write(tmp_path, "empty", C.EMPTY)
    assert g.foreign_gz_meta(p) is None
    assert g.read_foreign_gzip_file_to_device(p, 1024) is None


# ---------------------------------------------------------------------------
# whole reads
# ---------------------------------------------------------------------------

def _frames(tmp_path, tag, lo, hi):
    """Raw TFRecord frames of rows lo..hi, written by the project itself."""
    d = str(tmp_path / f"src_{tag}")
    rng = np.random.default_rng(lo)
    stf.write_tfrecord(
        {"x": np.arange(lo, hi, dtype=np.int64),
         "w": rng.integers(0, 7, hi - lo).astype(np.int64),
         "s": [f"row-{i % 13}" for i in range(lo, hi)]},
        d, engine="cpu")
    (f,) = P.list_data_files(d)
    with open(f, "rb") as fh:
        return fh.read()


def _rows(df):
    return sorted((r["x"], r["w"], r["s"]) for r in df.collect())


def _mixed_dir(tmp_path):
    out = str(tmp_path / "mix")
    os.makedirs(out)
    with open(os.path.join(out, "part-00000.tfrecord"), "wb") as f:
        f.write(_frames(tmp_path, "a", 0, 3000))
    with open(os.path.join(out, "part-00001.tfrecord.gz"), "wb") as f:
        f.write(P.compress_bytes(_frames(tmp_path, "b", 3000, 6000), "gzip"))
    raw = _frames(tmp_path, "c", 6000, 16000)
    with open(os.path.join(out, "part-00002.tfrecord.gz"), "wb") as f:
        # memLevel 3: many small dynamic blocks (at memLevel 1 zlib codes
        # real frames in fixed blocks, whose starts are not searched for)
        f.write(C.wrap(C.raw_deflate(raw, 6, 3), raw))
    raw = _frames(tmp_path, "d", 16000, 19000)
    import gzip
    with open(os.path.join(out, "part-00003.tfrecord.gz"), "wb") as f:
        f.write(gzip.compress(raw, 6))
    r1 = _frames(tmp_path, "e", 19000, 20000)
    r2 = _frames(tmp_path, "f", 20000, 21000)
    with open(os.path.join(out, "part-00004.tfrecord.gz"), "wb") as f:
        f.write(gzip.compress(r1, 6) + gzip.compress(r2, 6))  # two members
    return out


def test_group_read_matches_host(tmp_path, monkeypatch):
    g = _gpu_engine()
    monkeypatch.setenv("TFREC_GZ_FOREIGN_CHUNK", "2048")
    out = _mixed_dir(tmp_path)
    files = P.list_data_files(out)
    assert g.gz_device_meta(files[1]) is not None
    assert all(g.gz_device_meta(f) is None for f in files[2:])
    host = stf.read_tfrecord(out, engine="gpu", foreign_gzip="host")
    want = _rows(host)
    assert [r[0] for r in want] == list(range(21000))
    calls = []
    real = g._device_inflate_foreign_group

    def spy(data, items, device, chunk_bytes=None):
        ok = real(data, items, device, chunk_bytes)
        calls.append(([os.path.basename(it[0]) for it in items], ok,
                      [e[1] for e in g.last_foreign]))
        return ok

    monkeypatch.setattr(g, "_device_inflate_foreign_group", spy)
    dev = stf.read_tfrecord(out, engine="gpu", foreign_gzip="device")
    assert _rows(dev) == want
    assert dev.schema == host.schema  # both inferred
    # first attempt: all three foreign files in one launch, the two-member
    # one refused; second attempt: the two good ones, accepted in parallel
    names = [os.path.basename(f) for f in files]
    assert calls[0][0] == names[2:] and calls[0][1] == [True, True, False]
    assert calls[1][0] == names[2:4] and calls[1][1] == [True, True]
    assert calls[1][2][0] >= 20, calls  # live chunks of the small-block file
    assert len(calls) == 2
    nocrc = stf.read_tfrecord(out, engine="gpu", foreign_gzip="device",
                              verify_crc=False)
    assert _rows(nocrc) == want
    fluent = stf.session.read.option("engine", "gpu") \
        .option("foreignGzip", "device").load(out)
    assert _rows(fluent) == want
    # option unset: the foreign files stay on the host
    del calls[:]
    assert _rows(stf.read_tfrecord(out, engine="gpu")) == want
    assert calls == []


def test_refused_first_file_defers_inference_to_host(tmp_path):
    out = str(tmp_path / "two")
    os.makedirs(out)
    import gzip
    r1 = _frames(tmp_path, "a", 0, 500)
    r2 = _frames(tmp_path, "b", 500, 1000)
    with open(os.path.join(out, "part-00000.tfrecord.gz"), "wb") as f:
        f.write(gzip.compress(r1, 6) + gzip.compress(r2, 6))
    host = stf.read_tfrecord(out, engine="gpu", foreign_gzip="host")
    dev = stf.read_tfrecord(out, engine="gpu", foreign_gzip="device")
    assert _rows(dev) == _rows(host) and len(_rows(dev)) == 1000
    assert dev.schema == host.schema


def _outcome(fn):
    try:
        return ("rows", _rows(fn()))
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        return ("raises", type(e).__name__)


@pytest.mark.parametrize("damage", ["truncated", "bad_crc", "bad_isize",
                                    "bit_flip"])
def test_damaged_file_ends_as_on_host(tmp_path, damage):
    raw = _frames(tmp_path, "a", 0, 4000)
    gz = bytearray(C.wrap(C.raw_deflate(raw, 6, 3), raw))
    if damage == "truncated":
        gz = gz[:len(gz) // 2] + gz[-8:]
    elif damage == "bad_crc":
        gz[-8] ^= 0x01
    elif damage == "bad_isize":
        gz[-4] ^= 0x01
    else:
        gz[10 + (len(gz) - 18) // 2] ^= 0x10
    out = str(tmp_path / "bad")
    os.makedirs(out)
    with open(os.path.join(out, "part-00000.tfrecord.gz"), "wb") as f:
        f.write(bytes(gz))
    schema = stf.read_tfrecord(str(tmp_path / "src_a"), engine="cpu").schema
    host = _outcome(lambda: stf.read_tfrecord(
        out, schema=schema, engine="gpu", foreign_gzip="host"))
    dev = _outcome(lambda: stf.read_tfrecord(
        out, schema=schema, engine="gpu", foreign_gzip="device"))
    assert dev == host
    if damage == "bit_flip":
        assert host[0] == "raises"


def test_dataset_matches_host(tmp_path, monkeypatch):
    monkeypatch.setenv("TFREC_GZ_FOREIGN_CHUNK", "2048")
    from spark_tfrecord_amd.torch_data import TFRecordIterableDataset

    out = str(tmp_path / "ds")
    os.makedirs(out)
    for k, (lo, hi) in enumerate([(0, 4000), (4000, 6000)]):
        raw = _frames(tmp_path, str(k), lo, hi)
        with open(os.path.join(out, f"part-{k:05d}.tfrecord.gz"), "wb") as f:
            f.write(C.wrap(C.raw_deflate(raw, 6, 3 if k == 0 else 8), raw))
    schema = stf.read_tfrecord(str(tmp_path / "src_0"), engine="cpu").schema

    def values(mode):
        ds = TFRecordIterableDataset(out, schema=schema, engine="gpu",
                                     foreign_gzip=mode, prefetch=0)
        got = {}
        for item in ds:
            for k, v in item.items():
                got.setdefault(k, []).append(np.atleast_1d(v.cpu().numpy()))
        return {k: np.concatenate(v) for k, v in got.items()}

    g = _gpu_engine()
    seen = []
    real = g._device_inflate_foreign_group

    def spy(data, items, device, chunk_bytes=None):
        ok = real(data, items, device, chunk_bytes)
        seen.extend(g.last_foreign)
        return ok

    monkeypatch.setattr(g, "_device_inflate_foreign_group", spy)
    host = values("host")
    assert seen == []
    dev = values("device")
    assert len(seen) == 2 and all(e[3] == -1 for e in seen)
    assert seen[0][1] >= 10  # live chunks of the small-block shard
    assert host.keys() == dev.keys()
    for k in host:
        assert np.array_equal(host[k], dev[k]), k
    assert np.array_equal(np.sort(dev["x"]), np.arange(6000))
