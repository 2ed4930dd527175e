"""GPU tests of the shared host side of the multi-file reads in
engine/gpu.py: the one file upload (_upload_files), the one single-file
entry point (read_file_image), and a whole read that classifies each file
once (device_source) and hands the records on to read_files_to_batch."""

import gzip
import zlib

import numpy as np
import pytest

import snappy_cases as C
import spark_tfrecord_amd as stf
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P

pytestmark = pytest.mark.gpu


def _gpu_engine():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _put(path, blob):
    with open(path, "wb") as f:
        f.write(blob)
    return str(path)


# ---------------------------------------------------------------------------
# _upload_files
# ---------------------------------------------------------------------------

UPLOAD_SIZES = (0, 1, 4097, 3 * 4096 + 5)
UPLOAD_OFFSETS = (7, 100, 5000, 20001)  # gaps between every two files
UPLOAD_TOTAL = 40000


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "staged"])
def test_upload_files(tmp_path, monkeypatch, pinned):
    import torch

    g = _gpu_engine()
    rng = np.random.default_rng(5)
    blobs = [rng.integers(0, 256, n).astype(np.uint8) for n in UPLOAD_SIZES]
    paths = [_put(tmp_path / f"f{k}.bin", b.tobytes())
             for k, b in enumerate(blobs)]
    if not pinned:
        # no mapping can be pinned: every file takes the staged read, in
        # 4 KiB chunks, so the two larger files alternate both halves of
        # its staging buffer
        monkeypatch.setattr(_native, "file_mmap_pinned",
                            lambda path, n, writable: (0, False))
        monkeypatch.setattr(g, "_CHUNK", 4096)
    dst = torch.zeros(UPLOAD_TOTAL, dtype=torch.uint8, device="cuda")
    g._upload_files(dst, list(zip(paths, UPLOAD_SIZES, UPLOAD_OFFSETS)))
    torch.cuda.current_stream().synchronize()
    want = np.zeros(UPLOAD_TOTAL, np.uint8)
    for b, off in zip(blobs, UPLOAD_OFFSETS):
        want[off:off + b.size] = b
    got = dst.cpu().numpy()
    for b, off in zip(blobs, UPLOAD_OFFSETS):
        assert np.array_equal(got[off:off + b.size], b), off
    assert np.array_equal(got, want)  # and zero everywhere else


# ---------------------------------------------------------------------------
# read_file_image
# ---------------------------------------------------------------------------

RAW = C.example_image(300)
RAW2 = C.example_image(200)

# (file name, file image, foreign_gzip, on the device)
IMAGE_CASES = {
    "raw": ("a.tfrecord", RAW, False, True),
    "own_gzip": ("a.tfrecord.gz", P.compress_bytes(RAW, "gzip"), False, True),
    "other_gzip": ("a.tfrecord.gz", gzip.compress(RAW), True, True),
    "snappy": ("a.tfrecord.snappy", P.compress_bytes(RAW, "snappy"), False,
               True),
    "snappy_failed_walk": ("a.tfrecord.snappy", C.malformed_files()[0][1],
                           False, False),
    "deflate": ("a.tfrecord.deflate", zlib.compress(RAW), True, False),
    "empty_raw": ("a.tfrecord", b"", False, True),
    "empty_gzip": ("a.tfrecord.gz", b"", True, False),
    "empty_snappy": ("a.tfrecord.snappy", b"", False, True),
}


@pytest.mark.parametrize("name", list(IMAGE_CASES))
def test_read_file_image(tmp_path, name):
    g = _gpu_engine()
    fname, blob, foreign_gzip, on_device = IMAGE_CASES[name]
    p = _put(tmp_path / fname, blob)
    assert (g.device_source(p, foreign_gzip) is not None) == on_device
    dev = g.read_file_image(p, foreign_gzip)
    if on_device:
        assert dev is not None
        assert dev.cpu().numpy().tobytes() == P.decompress_file(p)
    else:
        assert dev is None


def _foreign_spy(g, monkeypatch):
    calls = []
    real = g._device_inflate_foreign_group

    def spy(data, items, device, chunk_bytes=None):
        ok = real(data, items, device, chunk_bytes)
        calls.append(([it[0] for it in items], ok))
        return ok

    monkeypatch.setattr(g, "_device_inflate_foreign_group", spy)
    return calls


def test_two_member_gzip_is_asked_and_refused(tmp_path, monkeypatch):
    g = _gpu_engine()
    p = _put(tmp_path / "a.tfrecord.gz",
             gzip.compress(RAW) + gzip.compress(RAW2))
    calls = _foreign_spy(g, monkeypatch)
    assert g.device_source(p, True).kind == "foreign"
    assert g.read_file_image(p, True) is None
    assert calls == [([p], [False])]


def test_foreign_gzip_off_never_reaches_the_inflater(tmp_path, monkeypatch):
    g = _gpu_engine()
    p = _put(tmp_path / "a.tfrecord.gz", gzip.compress(RAW))
    calls = _foreign_spy(g, monkeypatch)
    assert g.read_file_image(p) is None
    assert g.read_file_image(p, foreign_gzip=False) is None
    assert calls == []


# ---------------------------------------------------------------------------
# a whole read classifies each file once
# ---------------------------------------------------------------------------

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


def _rows(df):
    return [(r["x"], r["s"]) for r in df.collect()]


def test_each_file_is_classified_once(tmp_path, monkeypatch):
    g = _gpu_engine()
    out = tmp_path / "mix"
    out.mkdir()
    _put(out / "part-00000.tfrecord", _frames(tmp_path, "a", 0, 1000))
    _put(out / "part-00001.tfrecord.gz",
         P.compress_bytes(_frames(tmp_path, "b", 1000, 1800), "gzip"))
    _put(out / "part-00002.tfrecord.gz",
         gzip.compress(_frames(tmp_path, "c", 1800, 3000), 6))
    _put(out / "part-00003.tfrecord.snappy",
         P.compress_bytes(_frames(tmp_path, "d", 3000, 4000), "snappy"))
    classified = []
    groups = []
    real_source = g.device_source
    real_read = g.read_files_to_batch

    def source_spy(path, foreign_gzip=False):
        classified.append((path, foreign_gzip))
        return real_source(path, foreign_gzip)

    def read_spy(paths, *a, **k):
        groups.append(list(paths))
        return real_read(paths, *a, **k)

    monkeypatch.setattr(g, "device_source", source_spy)
    monkeypatch.setattr(g, "read_files_to_batch", read_spy)

    files = P.list_data_files(str(out))
    assert len(files) == 4
    dev = stf.read_tfrecord(str(out), engine="gpu", foreign_gzip="device")
    assert sorted(classified) == [(f, True) for f in files]
    assert groups == [files]
    want = stf.read_tfrecord(str(out), engine="cpu")
    assert dev.schema == want.schema
    assert _rows(dev) == _rows(want) and len(_rows(dev)) == 4000

    # a fifth file, which the device refuses: nobody is asked twice, and
    # the group is redone with the four records the reader already has
    _put(out / "part-00004.tfrecord.gz",
         gzip.compress(_frames(tmp_path, "e", 4000, 4300), 6)
         + gzip.compress(_frames(tmp_path, "f", 4300, 4500), 6))
    five = P.list_data_files(str(out))
    assert five[:4] == files and len(five) == 5
    del classified[:], groups[:]
    dev = stf.read_tfrecord(str(out), engine="gpu", foreign_gzip="device")
    assert sorted(classified) == [(f, True) for f in five]
    assert groups == [five, files]
    want = stf.read_tfrecord(str(out), engine="cpu")
    assert _rows(dev) == _rows(want) and len(_rows(dev)) == 4500
