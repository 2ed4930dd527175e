"""CPU tests of engine/gpu.py device_source, the one place that decides
where a file's bytes come from: which files it gives to which device
decoder, with what metadata and decompressed length, and which it leaves to
the host. The expectations are the rules each codec's read path follows,
written out per case; nothing here touches a device."""

import gzip
import zlib

import numpy as np
import pytest

import snappy_cases as C
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.engine import gpu as g
from spark_tfrecord_amd.io import paths as P

RAW = C.example_image(200)  # 200 small Example frames
RAW2 = C.example_image(120)
BAD_SNAPPY = C.malformed_files()[0][1]

# name -> (file name, file image, kind without foreign_gzip, kind with it);
# kind None = host bytes
CASES = {
    "raw": ("a.tfrecord", RAW, "raw", "raw"),
    "own_gzip": ("a.tfrecord.gz", P.compress_bytes(RAW, "gzip"),
                 "gzip", "gzip"),
    "other_gzip": ("a.tfrecord.gz", gzip.compress(RAW), None, "foreign"),
    "two_members": ("a.tfrecord.gz", gzip.compress(RAW) + gzip.compress(RAW2),
                    None, "foreign"),
    "snappy": ("a.tfrecord.snappy", P.compress_bytes(RAW, "snappy"),
               "snappy", "snappy"),
    "snappy_failed_walk": ("a.tfrecord.snappy", BAD_SNAPPY, None, None),
    "deflate": ("a.tfrecord.deflate", zlib.compress(RAW), None, None),
    "empty_raw": ("a.tfrecord", b"", "raw", "raw"),
    "empty_gzip": ("a.tfrecord.gz", b"", None, None),
    "empty_snappy": ("a.tfrecord.snappy", b"", "snappy", "snappy"),
    "empty_deflate": ("a.tfrecord.deflate", b"", None, None),
}

META_OF = {"raw": lambda p: None, "gzip": g.gz_device_meta,
           "foreign": g.foreign_gz_meta, "snappy": g.snappy_device_meta}


@pytest.fixture(autouse=True)
def kernels_present(monkeypatch):
    monkeypatch.setattr(_native, "HAS_GPU_KERNELS", True, raising=False)
    monkeypatch.delenv("TFREC_SNAPPY", raising=False)


def _write(tmp_path, name):
    fname, blob = CASES[name][:2]
    p = str(tmp_path / fname)
    with open(p, "wb") as f:
        f.write(blob)
    return p


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)
                and a.dtype == b.dtype and np.array_equal(a, b))
    if isinstance(a, (tuple, list)):
        return (type(a) is type(b) and len(a) == len(b)
                and all(_same(x, y) for x, y in zip(a, b)))
    return a == b


@pytest.mark.parametrize("foreign_gzip", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_classification(tmp_path, name, foreign_gzip):
    p = _write(tmp_path, name)
    kind = CASES[name][3 if foreign_gzip else 2]
    src = g.device_source(p, foreign_gzip)
    if kind is None:
        assert src is None
        return
    assert src is not None and src.kind == kind
    assert _same(src.meta, META_OF[kind](p))
    assert (src.meta is None) == (kind == "raw")
    if name == "two_members":
        # the trailer read is the last member's: its ISIZE, not the file's
        # length (the inflater refuses the file on that mismatch)
        assert src.nbytes == len(RAW2) != len(P.decompress_file(p))
    else:
        assert src.nbytes == len(P.decompress_file(p))
    with pytest.raises(AttributeError):
        src.kind = "raw"  # immutable


def test_default_leaves_other_writers_gzip_to_the_host(tmp_path):
    assert g.device_source(_write(tmp_path, "other_gzip")) is None


def test_segment_table_is_asked_before_the_foreign_header(tmp_path):
    p = _write(tmp_path, "own_gzip")
    assert g.foreign_gz_meta(p) is not None  # eligible there too
    assert g.device_source(p, True).kind == "gzip"


def test_snappy_knob(tmp_path, monkeypatch):
    p = _write(tmp_path, "snappy")
    monkeypatch.setenv("TFREC_SNAPPY", "host")
    assert g.device_source(p) is None
    assert g.device_source(p, True) is None
    monkeypatch.setenv("TFREC_SNAPPY", "neither")
    with pytest.raises(ValueError, match="TFREC_SNAPPY"):
        g.device_source(p)


def test_snappy_chunk_cap_is_read_at_call_time(tmp_path, monkeypatch):
    p = _write(tmp_path, "snappy")
    chunk = int(g.device_source(p).meta[0][:, 3].max())
    monkeypatch.setattr(g, "SNAPPY_MAX_CHUNK_RAW", chunk - 1)
    assert g.device_source(p) is None
    monkeypatch.setattr(g, "SNAPPY_MAX_CHUNK_RAW", chunk)
    assert g.device_source(p).nbytes == len(RAW)


@pytest.mark.parametrize("foreign_gzip", [False, True])
def test_without_kernels_every_compressed_file_is_for_the_host(
        tmp_path, monkeypatch, foreign_gzip):
    monkeypatch.setattr(_native, "HAS_GPU_KERNELS", False, raising=False)
    for name, (fname, _, _, _) in CASES.items():
        d = tmp_path / name
        d.mkdir()
        src = g.device_source(_write(d, name), foreign_gzip)
        if fname.endswith(".tfrecord"):
            assert src is not None and src.kind == "raw"
        else:
            assert src is None, name
