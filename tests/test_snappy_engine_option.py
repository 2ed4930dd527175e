"""The snappy_engine write option (io/writer.py), as far as it goes without
a GPU: value checking, the TFREC_SNAPPY_ENGINE default, and what it is
ignored for. tests/test_gpu_snappy_enc.py covers the device path itself."""

import logging

import numpy as np
import pytest

import spark_tfrecord_amd as stf
from spark_tfrecord_amd.io import paths as P
from spark_tfrecord_amd.io.writer import _resolve_snappy_engine

DATA = {"x": np.arange(50, dtype=np.int64)}


def test_device_with_cpu_engine_raises(tmp_sandbox):
    out = str(tmp_sandbox / "o")
    with pytest.raises(ValueError, match="GPU engine"):
        stf.write_tfrecord(DATA, out, engine="cpu", codec="snappy",
                           snappy_engine="device")
    with pytest.raises(ValueError, match="GPU engine"):
        stf.session.createDataFrame(DATA).write.option("engine", "cpu") \
            .option("codec", "snappy").option("snappyEngine", "device") \
            .save(out)


def test_unknown_value_raises(tmp_sandbox):
    with pytest.raises(ValueError, match="snappy engine"):
        stf.write_tfrecord(DATA, str(tmp_sandbox / "o"), engine="cpu",
                           codec="snappy", snappy_engine="fpga")
    with pytest.raises(ValueError, match="snappy engine"):
        stf.session.createDataFrame(DATA).write.option("engine", "cpu") \
            .option("codec", "snappy").option("snappyEngine", "fpga") \
            .save(str(tmp_sandbox / "o"))


def test_env_default_is_for_gpu_engine_only(tmp_sandbox, monkeypatch):
    monkeypatch.setenv("TFREC_SNAPPY_ENGINE", "device")
    out = str(tmp_sandbox / "o")
    stf.write_tfrecord(DATA, out, engine="cpu", codec="snappy")  # no error
    (f,) = P.list_data_files(out)
    assert f.endswith(".snappy")
    with open(f, "rb") as fh:
        assert P.snappy_walk(fh.read(), f)[1] > 0
    got = stf.read_tfrecord(out, engine="cpu").sort("x").collect()
    assert [r["x"] for r in got] == list(range(50))
    assert _resolve_snappy_engine(None, "gpu", "snappy") is True
    assert _resolve_snappy_engine(None, "cpu", "snappy") is False
    assert _resolve_snappy_engine("host", "gpu", "snappy") is False


def test_default_and_ignored_codecs(monkeypatch):
    monkeypatch.delenv("TFREC_SNAPPY_ENGINE", raising=False)
    assert _resolve_snappy_engine(None, "gpu", "snappy") is False
    assert _resolve_snappy_engine("device", "gpu", "snappy") is True
    assert _resolve_snappy_engine("Device", "gpu", "snappy") is True
    for codec in ("gzip", "deflate", None):
        assert _resolve_snappy_engine("device", "gpu", codec) is False


@pytest.mark.parametrize("codec", ["gzip", "deflate", None])
def test_ignored_for_other_codecs(tmp_sandbox, codec):
    out = str(tmp_sandbox / f"c{codec}")
    stf.write_tfrecord(DATA, out, engine="cpu", codec=codec,
                       snappy_engine="host")
    got = stf.read_tfrecord(out, engine="cpu").sort("x").collect()
    assert [r["x"] for r in got] == list(range(50))
    # the value is still checked, and "device" still needs the GPU engine
    with pytest.raises(ValueError, match="GPU engine"):
        stf.write_tfrecord(DATA, out, engine="cpu", codec=codec,
                           snappy_engine="device", mode="overwrite")


def test_block_above_the_device_cap_goes_to_the_host(monkeypatch, caplog):
    monkeypatch.setattr(P, "_SNAPPY_BLOCK", (1 << 20) + 1)
    with caplog.at_level(logging.WARNING):
        assert _resolve_snappy_engine("device", "gpu", "snappy") is False
    assert "TFREC_SNAPPY_BLOCK" in caplog.text and "host" in caplog.text
    monkeypatch.setattr(P, "_SNAPPY_BLOCK", 1 << 20)
    assert _resolve_snappy_engine("device", "gpu", "snappy") is True
