"""CPU tests of the speculative foreign-gzip inflater core
(csrc/inflate_spec_core.h) through its host build,
`_native.host_inflate_foreign`, and of the `foreign_gzip` read option as far
as it goes without a GPU. tests/test_gpu_inflate_foreign.py runs the same
cases through the kernels."""

import gzip

import numpy as np
import pytest

import foreign_gz_cases as C
import spark_tfrecord_amd as stf
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.engine import gpu as gpu_engine
from spark_tfrecord_amd.io.reader import _resolve_foreign_gzip

MAIN = C.main_cases()
VARIANTS = C.variant_cases()
REJECTED = C.rejected_cases()


def _strides(gz, own):
    return sorted({own, 1024, 4096, 32768, len(gz) + 1})


@pytest.mark.parametrize("name,gz,data,stride,cond", MAIN,
                         ids=[c[0] for c in MAIN])
def test_main_cases(name, gz, data, stride, cond):
    assert gzip.decompress(gz) == data
    for s in _strides(gz, stride):
        out, stats = _native.host_inflate_foreign(gz, s)
        assert out == data, f"stride {s}"
        assert stats["live_chunks"] >= 1
        if s > len(gz):
            assert stats["live_chunks"] == 1 and stats["candidates"] == 0
    out, stats = _native.host_inflate_foreign(gz, stride)
    kind, n = cond
    if kind == "min":
        assert stats["live_chunks"] >= n, stats
    else:
        assert stats["live_chunks"] == n, stats
    # every start found is either on the chain or counted as discarded
    assert (stats["live_chunks"] - 1 + stats["discarded"]
            == stats["candidates"])


def test_window_chain_is_exercised():
    name, gz, data, stride, _ = MAIN[0]
    assert name == "dyn_small_blocks"
    _, stats = _native.host_inflate_foreign(gz, stride)
    assert stats["marker_symbols"] > 0


def test_fixed_mix_keeps_dynamic_blocks():
    name, gz, data, _, _ = [c for c in MAIN if c[0] == "fixed_mix"][0]
    # a start is only ever found at a non-final dynamic block's head
    _, stats = _native.host_inflate_foreign(gz, 1024)
    assert stats["candidates"] >= 5, stats


@pytest.mark.parametrize("name,gz,data,stride", VARIANTS,
                         ids=[c[0] for c in VARIANTS])
def test_headers_and_edges(name, gz, data, stride):
    assert gzip.decompress(gz) == data
    for s in _strides(gz, stride):
        out, _ = _native.host_inflate_foreign(gz, s)
        assert out == data, f"stride {s}"


def test_window_edge_reaches_across_chunks():
    gz, data = C.window_edge_case()
    out, stats = _native.host_inflate_foreign(gz, 1024)
    assert out == data
    assert stats["live_chunks"] > 4 and stats["marker_symbols"] > 0


def test_empty_payload_is_ineligible():
    with pytest.raises(RuntimeError, match="eligible"):
        _native.host_inflate_foreign(C.EMPTY, 1024)
    assert gpu_engine._foreign_gz_parse(C.EMPTY, C.EMPTY[-8:],
                                        len(C.EMPTY)) is None


@pytest.mark.parametrize("name,gz,host", REJECTED,
                         ids=[c[0] for c in REJECTED])
def test_rejections(name, gz, host):
    for s in (1024, 2048, len(gz) + 1):
        with pytest.raises(RuntimeError):
            _native.host_inflate_foreign(gz, s)
    if host is not None:
        assert gzip.decompress(gz) == host
    else:
        with pytest.raises(Exception):
            gzip.decompress(gz)


def test_header_walk():
    name, gz, data, _ = VARIANTS[0]
    assert name == "hdr_all"
    body_off, body_len, crc, isize = gpu_engine._foreign_gz_parse(
        gz, gz[-8:], len(gz))
    assert isize == len(data)
    assert body_off + body_len + 8 == len(gz)
    import zlib
    assert zlib.decompress(gz[body_off:body_off + body_len], -15) == data
    assert crc == zlib.crc32(data)
    # ineligible: not deflate, too short, reserved flag bits
    bad_cm = gz[:2] + b"\x07" + gz[3:]
    assert gpu_engine._foreign_gz_parse(bad_cm, gz[-8:], len(gz)) is None
    assert gpu_engine._foreign_gz_parse(gz[:3] + b"\xe0" + gz[4:], gz[-8:],
                                        len(gz)) is None


def test_read_option_resolution(tmp_sandbox, monkeypatch):
    monkeypatch.delenv("TFREC_GZ_FOREIGN", raising=False)
    assert _resolve_foreign_gzip(None, "gpu") is False
    assert _resolve_foreign_gzip("device", "gpu") is True
    assert _resolve_foreign_gzip("Device", "gpu") is True
    assert _resolve_foreign_gzip("host", "gpu") is False
    assert _resolve_foreign_gzip("host", "cpu") is False
    monkeypatch.setenv("TFREC_GZ_FOREIGN", "device")
    assert _resolve_foreign_gzip(None, "gpu") is True
    assert _resolve_foreign_gzip(None, "cpu") is False  # env ignored
    assert _resolve_foreign_gzip("host", "gpu") is False
    with pytest.raises(ValueError, match="foreign gzip"):
        _resolve_foreign_gzip("fpga", "gpu")
    with pytest.raises(ValueError, match="GPU engine"):
        _resolve_foreign_gzip("device", "cpu")
    monkeypatch.setenv("TFREC_GZ_FOREIGN", "fpga")
    with pytest.raises(ValueError, match="foreign gzip"):
        _resolve_foreign_gzip(None, "gpu")


def test_read_option_on_cpu_engine(tmp_sandbox, monkeypatch):
    out = str(tmp_sandbox / "o")
    stf.write_tfrecord({"x": np.arange(50, dtype=np.int64)}, out,
                       engine="cpu")
    with pytest.raises(ValueError, match="GPU engine"):
        stf.read_tfrecord(out, engine="cpu", foreign_gzip="device")
    with pytest.raises(ValueError, match="GPU engine"):
        stf.session.read.option("engine", "cpu") \
            .option("foreignGzip", "device").load(out)
    with pytest.raises(ValueError, match="foreign gzip"):
        stf.read_tfrecord(out, engine="cpu", foreign_gzip="fpga")
    monkeypatch.setenv("TFREC_GZ_FOREIGN", "device")
    got = stf.read_tfrecord(out, engine="cpu").sort("x").collect()
    assert [r["x"] for r in got] == list(range(50))
    got = stf.read_tfrecord(out, engine="cpu", foreign_gzip="host").collect()
    assert len(got) == 50


def test_dataset_option_value_checked(tmp_sandbox):
    from spark_tfrecord_amd.torch_data import TFRecordIterableDataset

    out = str(tmp_sandbox / "o")
    stf.write_tfrecord({"x": np.arange(5, dtype=np.int64)}, out, engine="cpu")
    with pytest.raises(ValueError, match="foreign gzip"):
        TFRecordIterableDataset(out, engine="cpu", foreign_gzip="fpga")
    ds = TFRecordIterableDataset(out, engine="cpu", foreign_gzip="device")
    with pytest.raises(ValueError, match="GPU engine"):
        next(iter(ds))
