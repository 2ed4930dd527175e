"""The sliced file write where the file's mapping cannot be registered: the
slices go from pinned staging into the (unregistered) mapping through the IO
pool, or, with the knob off or no mapping at all, through pwrite(). Every
route must leave the host codec's bytes in a file of exactly that size. On a
platform that registers the mapping these cases run the DMA path instead and
still check the same bytes."""

import os

import numpy as np
import pytest

from spark_tfrecord_amd.engine import cpu as cpu_engine

_cache = {}


def _case(rows):
    """(host batch, host image), made once per row count."""
    if rows not in _cache:
        from bench import make_batch
        b = make_batch(rows, seed=5)
        _cache[rows] = (b, bytes(cpu_engine.encode_batch(b, "Example")))
    return _cache[rows]


def test_memcpy_parallel_copies_every_byte():
    # sizes around the pool's minimum span (256 KiB) and its 8-way split
    from spark_tfrecord_amd import _native
    rng = np.random.default_rng(0)
    for n in (0, 1, (256 << 10) - 1, 256 << 10, (256 << 10) + 1,
              8 * (256 << 10) + 13, 5_000_001):
        src = rng.integers(0, 256, n + 16, dtype=np.uint8)
        dst = np.full(n + 32, 0xA5, np.uint8)
        _native.memcpy_parallel(dst.ctypes.data + 8, src.ctypes.data + 3, n)
        assert np.array_equal(dst[8:8 + n], src[3:3 + n])
        assert (dst[:8] == 0xA5).all() and (dst[8 + n:] == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["mapped", "pwrite", "no-mapping"])
@pytest.mark.parametrize("slices", [1, 5, 64])
@pytest.mark.parametrize("rows", [1, 3, 300])
def test_sliced_write_routes(tmp_path, monkeypatch, rows, slices, route):
    from spark_tfrecord_amd import _native
    from spark_tfrecord_amd.engine import gpu as g
    b, want = _case(rows)
    monkeypatch.setattr(g, "_STAGED_MAPPED_WRITE", route == "mapped")
    if route == "no-mapping":
        monkeypatch.setattr(_native, "file_mmap_pinned",
                            lambda path, n, writable: (0, False))
    path = str(tmp_path / "w.tfrecord")
    dev = g.batch_to_device(b)
    assert g.write_batch_to_file(dev, path, "Example", slices=slices) == len(want)
    assert os.path.getsize(path) == len(want)
    with open(path, "rb") as f:
        assert f.read() == want


@pytest.mark.gpu
@pytest.mark.parametrize("mapped", [True, False])
@pytest.mark.parametrize("before", [-50, 0, 100])
def test_write_over_an_existing_file(tmp_path, monkeypatch, mapped, before):
    # a shorter, an equal and a longer file is there already; the second and
    # third write find the mapping cached, the third another batch's bytes
    from spark_tfrecord_amd.engine import gpu as g
    b, want = _case(300)
    monkeypatch.setattr(g, "_STAGED_MAPPED_WRITE", mapped)
    path = str(tmp_path / "w.tfrecord")
    with open(path, "wb") as f:
        f.write(b"\xa5" * (len(want) + before))
    dev = g.batch_to_device(b)
    for _ in range(2):
        assert g.write_batch_to_file(dev, path, "Example", slices=5) == len(want)
        with open(path, "rb") as f:
            assert f.read() == want
    b2, want2 = _case(3)
    assert g.write_batch_to_file(g.batch_to_device(b2), path, "Example") == len(want2)
    with open(path, "rb") as f:
        assert f.read() == want2


@pytest.mark.gpu
def test_mapped_write_reads_back(tmp_path, monkeypatch):
    from spark_tfrecord_amd.engine import gpu as g
    b, want = _case(300)
    monkeypatch.setattr(g, "_STAGED_MAPPED_WRITE", True)
    path = str(tmp_path / "rt.tfrecord")
    g.write_batch_to_file(g.batch_to_device(b), path, "Example")
    got = g.batch_to_host(g.read_file_to_batch_pipelined(path, b.schema,
                                                         "Example", True))
    for a, c in zip(got.columns, b.columns):
        assert np.array_equal(np.asarray(a.values), np.asarray(c.values))
        assert np.array_equal(np.asarray(a.row_off), np.asarray(c.row_off))
