"""The gzip_engine write option (io/writer.py), as far as it goes without a
GPU: value checking, the TFREC_GZ_ENGINE default, and what it is ignored
for. tests/test_gpu_deflate.py covers the device path itself."""

import numpy as np
import pytest

import spark_tfrecord_amd as stf
from spark_tfrecord_amd.io import paths as P
from spark_tfrecord_amd.io.writer import _resolve_gzip_engine

DATA = {"x": np.arange(50, dtype=np.int64)}


def test_device_with_cpu_engine_raises(tmp_sandbox):
    out = str(tmp_sandbox / "o")
    with pytest.raises(ValueError, match="GPU engine"):
        stf.write_tfrecord(DATA, out, engine="cpu", codec="gzip",
                           gzip_engine="device")
    with pytest.raises(ValueError, match="GPU engine"):
        stf.session.createDataFrame(DATA).write.option("engine", "cpu") \
            .option("codec", "gzip").option("gzipEngine", "device").save(out)


def test_unknown_value_raises(tmp_sandbox):
    with pytest.raises(ValueError, match="gzip engine"):
        stf.write_tfrecord(DATA, str(tmp_sandbox / "o"), engine="cpu",
                           codec="gzip", gzip_engine="fpga")


def test_env_default_is_for_gpu_engine_only(tmp_sandbox, monkeypatch):
    monkeypatch.setenv("TFREC_GZ_ENGINE", "device")
    out = str(tmp_sandbox / "o")
    stf.write_tfrecord(DATA, out, engine="cpu", codec="gzip")  # no error
    assert P.parse_gz_segments_file(P.list_data_files(out)[0]) is not None
    got = stf.read_tfrecord(out, engine="cpu").sort("x").collect()
    assert [r["x"] for r in got] == list(range(50))
    assert _resolve_gzip_engine(None, "gpu", "gzip") is True
    assert _resolve_gzip_engine(None, "cpu", "gzip") is False
    assert _resolve_gzip_engine("host", "gpu", "gzip") is False


def test_default_and_ignored_codecs(monkeypatch):
    monkeypatch.delenv("TFREC_GZ_ENGINE", raising=False)
    assert _resolve_gzip_engine(None, "gpu", "gzip") is False
    assert _resolve_gzip_engine("device", "gpu", "gzip") is True
    assert _resolve_gzip_engine("Device", "gpu", "gzip") is True
    assert _resolve_gzip_engine("device", "gpu", "deflate") is False
    assert _resolve_gzip_engine("device", "gpu", None) is False
