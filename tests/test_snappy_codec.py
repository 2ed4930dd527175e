"""CPU tests of the Snappy codec's host side: the codec names, the Hadoop
block container (io/paths.py snappy_walk) written and read, and every
entry point that takes a codec or reads by extension."""

import os
import struct

import numpy as np
import pyarrow as pa
import pytest

import snappy_cases as C
import spark_tfrecord_amd as stf
from spark_tfrecord_amd.io import paths as P

FILES = C.valid_files()
BAD_FILES = C.malformed_files()
BAD_CHUNKS = C.malformed_chunks()


def _write(tmp_path, name, blob):
    p = str(tmp_path / f"{name}.tfrecord.snappy")
    with open(p, "wb") as f:
        f.write(blob)
    return p


def _blocks(img):
    """[(raw_len, [comp_len, ...])] of an image, walked with struct alone
    (independently of snappy_walk; one chunk per block expected)."""
    out = []
    pos = 0
    while pos < len(img):
        raw_len, comp_len = struct.unpack_from(">II", img, pos)
        out.append((raw_len, comp_len))
        pos += 8 + comp_len
    assert pos == len(img)
    return out


@pytest.mark.parametrize("name", ["snappy", "Snappy", " SNAPPY ",
                                  "org.apache.hadoop.io.compress.SnappyCodec",
                                  "ORG.APACHE.HADOOP.IO.COMPRESS.SNAPPYCODEC"])
def test_aliases(name):
    assert P.normalize_codec(name) == "snappy"


def test_extension():
    assert P.codec_extension("snappy") == ".snappy"
    assert P.codec_from_path("/x/part-00000-ab.tfrecord.snappy") == "snappy"
    assert P.part_file_name(3, "snappy", "j").endswith(".tfrecord.snappy")
    with pytest.raises(ValueError):
        P.normalize_codec("snappy2")


@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 65537, 200_001])
def test_bytes_round_trip(tmp_path, n):
    data = np.random.default_rng(n).integers(97, 110, n).astype(
        np.uint8).tobytes()
    img = P.compress_bytes(data, "snappy")
    if n == 0:
        assert img == b""
    blocks = _blocks(img)
    assert all(0 < raw <= 65536 for raw, _ in blocks)  # none empty
    assert sum(raw for raw, _ in blocks) == n
    assert len(blocks) == -(-n // 65536)
    assert P.decompress_file(_write(tmp_path, f"rt{n}", img)) == data


def test_block_size_knob(monkeypatch):
    monkeypatch.setattr(P, "_SNAPPY_BLOCK", 1000)
    data = bytes(range(256)) * 10
    blocks = _blocks(P.compress_bytes(data, "snappy"))
    assert [raw for raw, _ in blocks] == [1000, 1000, 560]
    assert P.snappy_decompress(P.compress_bytes(data, "snappy"), "x") == data


def test_compress_from_pool_worker():
    """compress_bytes runs on shared_pool() workers (io/writer.py): with
    every worker busy compressing, none may wait for the pool itself."""
    pool = P.shared_pool()
    data = b"pool-" * 40000
    futs = [pool.submit(P.compress_bytes, data, "snappy")
            for _ in range(128)]  # the pool has at most 32 workers
    for f in futs:
        assert P.snappy_decompress(f.result(timeout=60), "x") == data


@pytest.mark.parametrize("name,img,want", FILES, ids=[f[0] for f in FILES])
def test_hand_built_files_read_back(tmp_path, name, img, want):
    assert P.decompress_file(_write(tmp_path, name, img)) == want
    chunks, total = P.snappy_walk(img, name)
    assert total == len(want)
    assert sum(c[3] for c in chunks) == total
    if name == "one_block_three_chunks":
        assert len(chunks) == 3
    if name == "block_256k":
        assert [c[3] for c in chunks] == [256 << 10]


@pytest.mark.parametrize("name,img", BAD_FILES, ids=[f[0] for f in BAD_FILES])
def test_malformed_file_raises(tmp_path, name, img):
    p = _write(tmp_path, name, img)
    with pytest.raises(ValueError, match=r"(?s)" + name + r".*block 1"):
        P.decompress_file(p)


@pytest.mark.parametrize("name,comp,expect_len,cause", BAD_CHUNKS,
                         ids=[c[0] for c in BAD_CHUNKS])
def test_malformed_chunk_in_file_raises(tmp_path, name, comp, expect_len,
                                        cause):
    img = struct.pack(">II", expect_len, len(comp)) + comp
    p = _write(tmp_path, name, img)
    with pytest.raises(ValueError, match=name):
        P.decompress_file(p)


def test_preamble_beyond_block_raises(tmp_path):
    comp, want = C.library_chunks()[2][1:]
    img = struct.pack(">II", len(want) - 1, len(comp)) + comp
    with pytest.raises(ValueError, match="block 0"):
        P.decompress_file(_write(tmp_path, "short_block", img))


# ---------------------------------------------------------------------------
# the public entry points
# ---------------------------------------------------------------------------

def _example(n=500):
    rng = np.random.default_rng(5)
    return pa.table({
        "id": np.arange(n, dtype=np.int64),
        "w": rng.random(n).astype(np.float32),
        "s": [f"name-{i % 17}" for i in range(n)],
        "part": [i % 3 for i in range(n)],
    })


def _sorted_rows(df, key="id"):
    return sorted(df.collect(), key=lambda r: r[key])


def _snappy_files(out):
    files = P.list_data_files(out)
    assert files and all(f.endswith(".tfrecord.snappy") for f in files)
    return files


def test_example_round_trip(tmp_path):
    out = str(tmp_path / "ex")
    t = _example()
    stf.write_tfrecord(t, out, codec="snappy", engine="cpu", num_shards=2)
    assert len(_snappy_files(out)) == 2
    df = stf.read_tfrecord(out, engine="cpu")
    rows = _sorted_rows(df)
    assert [r["id"] for r in rows] == list(range(500))
    assert [r["s"] for r in rows] == t.column("s").to_pylist()
    assert np.allclose([r["w"] for r in rows], t.column("w").to_numpy())


def test_sequence_example_round_trip(tmp_path):
    out = str(tmp_path / "se")
    schema = stf.StructType([
        stf.StructField("id", stf.LongType(), True),
        stf.StructField("rag", stf.ArrayType(stf.ArrayType(stf.FloatType())),
                        True),
    ])
    data = {"id": list(range(500)),
            "rag": [[[float(i), 2.0], [3.0]] if i % 2 else [[4.0]]
                    for i in range(500)]}
    stf.write_tfrecord(data, out, record_type="SequenceExample",
                       schema=schema, codec="snappy", engine="cpu")
    _snappy_files(out)
    rows = _sorted_rows(stf.read_tfrecord(out, record_type="SequenceExample",
                                          engine="cpu"))
    assert [r["rag"] for r in rows] == data["rag"]


def test_byte_array_round_trip(tmp_path):
    out = str(tmp_path / "ba")
    payloads = [bytes([i % 251]) * (i % 40) for i in range(500)]
    t = pa.table({"byteArray": pa.array(payloads, type=pa.large_binary())})
    stf.write_tfrecord(t, out, record_type="ByteArray", codec="snappy",
                       engine="cpu")
    _snappy_files(out)
    df = stf.read_tfrecord(out, record_type="ByteArray", engine="cpu")
    assert [r["byteArray"] for r in df.collect()] == payloads


def test_partition_by(tmp_path):
    out = str(tmp_path / "parts")
    stf.write_tfrecord(_example(), out, codec="snappy", engine="cpu",
                       partition_by=["part"])
    files = _snappy_files(out)
    assert {os.path.basename(os.path.dirname(f)) for f in files} == \
        {"part=0", "part=1", "part=2"}
    rows = _sorted_rows(stf.read_tfrecord(out, engine="cpu"))
    assert [r["id"] for r in rows] == list(range(500))
    assert [r["part"] for r in rows] == [i % 3 for i in range(500)]


def test_fluent_codec_option(tmp_path):
    out = str(tmp_path / "fluent")
    df = stf.read_tfrecord(_plain(tmp_path), engine="cpu")
    df.write.option("engine", "cpu").option(
        "codec", "org.apache.hadoop.io.compress.SnappyCodec").save(out)
    _snappy_files(out)
    back = stf.session.read.option("engine", "cpu").load(out)
    assert _sorted_rows(back) == _sorted_rows(df)


def _plain(tmp_path):
    src = str(tmp_path / "plain")
    if not os.path.isdir(src):
        stf.write_tfrecord(_example(), src, engine="cpu")
    return src


def test_distributed_writer_single_process(tmp_path):
    from spark_tfrecord_amd.parallel import write_tfrecord_distributed

    out = str(tmp_path / "dist")
    write_tfrecord_distributed(_example(), out, codec="snappy")
    _snappy_files(out)
    assert stf.read_tfrecord(out, engine="cpu").count() == 500


def test_shard_writer_matches_one_shot(tmp_path, monkeypatch):
    monkeypatch.setattr(P, "_SNAPPY_BLOCK", 4096)  # several blocks + a tail
    t = _example()
    path = str(tmp_path / "sw" / "part-00000.tfrecord.snappy")
    with stf.ShardWriter(path, codec="snappy", engine="cpu") as w:
        for lo, hi in ((0, 100), (100, 350), (350, 500)):
            w.write(t.slice(lo, hi - lo))
    one = str(tmp_path / "one")
    stf.write_tfrecord(t, one, codec="snappy", engine="cpu")
    (f,) = _snappy_files(one)
    with open(path, "rb") as a, open(f, "rb") as b:
        img = a.read()
        assert img == b.read()  # the same blocks, the tail flushed on close
    blocks = _blocks(img)
    assert len(blocks) > 3 and all(0 < raw <= 4096 for raw, _ in blocks)
    assert _sorted_rows(stf.read_tfrecord(path, engine="cpu")) == \
        _sorted_rows(stf.read_tfrecord(one, engine="cpu"))


def test_shard_writer_without_rows_is_empty_file(tmp_path):
    path = str(tmp_path / "sw0" / "part-00000.tfrecord.snappy")
    stf.ShardWriter(path, codec="snappy", engine="cpu").close()
    assert os.path.getsize(path) == 0
    assert P.decompress_file(path) == b""


def test_count_and_validate(tmp_path):
    out = str(tmp_path / "cv")
    stf.write_tfrecord(_example(), out, codec="snappy", engine="cpu",
                       num_shards=2)
    assert stf.count_tfrecord(out, engine="cpu") == 500
    rep = stf.validate_tfrecord(out, engine="cpu")
    assert rep.ok and rep.records == 500 and len(rep.files) == 2
    # a flipped payload byte is a CRC error of the frame, not of the codec
    (f0, _f1) = _snappy_files(out)
    raw = bytearray(P.decompress_file(f0))
    raw[20] ^= 0xFF
    with open(f0, "wb") as f:
        f.write(P.compress_bytes(bytes(raw), "snappy"))
    rep = stf.validate_tfrecord(out, engine="cpu")
    assert not rep.ok and [x.ok for x in rep.files] == [False, True]
    # a broken container is reported, not raised
    with open(f0, "wb") as f:
        f.write(BAD_FILES[2][1])
    rep = stf.validate_tfrecord(out, engine="cpu")
    assert not rep.ok and "snappy block" in rep.files[0].error


def test_schema_inference_reads_snappy(tmp_path):
    out = str(tmp_path / "inf")
    stf.write_tfrecord(_example(), out, codec="snappy", engine="cpu")
    plain = stf.read_tfrecord(_plain(tmp_path), engine="cpu")
    assert stf.read_tfrecord(out, engine="cpu").schema == plain.schema


def test_cli_convert(tmp_path, capsys):
    from spark_tfrecord_amd.__main__ import main

    dst = str(tmp_path / "conv")
    assert main(["--engine", "cpu", "convert", _plain(tmp_path), dst,
                 "--codec", "snappy"]) == 0
    assert "wrote 500 records" in capsys.readouterr().out
    _snappy_files(dst)
    assert main(["--engine", "cpu", "count", dst]) == 0
    assert capsys.readouterr().out.strip() == "500"
    back = str(tmp_path / "back")
    assert main(["--engine", "cpu", "convert", dst, back]) == 0
    assert _sorted_rows(stf.read_tfrecord(back, engine="cpu")) == \
        _sorted_rows(stf.read_tfrecord(_plain(tmp_path), engine="cpu"))


@pytest.mark.parametrize("mode", ["device", "host"])
def test_knob_is_harmless_on_cpu_engine(tmp_path, monkeypatch, mode):
    monkeypatch.setenv("TFREC_SNAPPY", mode)
    out = str(tmp_path / "knob")
    stf.write_tfrecord(_example(), out, codec="snappy", engine="cpu")
    assert stf.read_tfrecord(out, engine="cpu").count() == 500
    assert stf.count_tfrecord(out, engine="cpu") == 500
