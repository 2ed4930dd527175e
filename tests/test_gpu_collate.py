"""GPU tier of the batch collation: collate_rows_kernel against the host run
of the same core on every case of collate_cases.py, and
TFRecordBatchDataset(engine="gpu") against engine="cpu". Nothing here hands
the launcher a selection it would have to reject; those are refused on the
host and tested in test_collate_core.py."""

import numpy as np
import pytest
import torch

import spark_tfrecord_amd as stf
from spark_tfrecord_amd.collate import (STATUS_CLEAN, Collator, FixedLen,
                                        Padded, Padded2D, collate_batch)
from spark_tfrecord_amd.torch_data import TFRecordBatchDataset

import collate_cases as C

pytestmark = pytest.mark.gpu


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same(got: dict, want: dict):
    assert set(got) == set(want)
    for k in want:
        g, w = bits(got[k]), bits(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert np.array_equal(g, w), k


def to_device(sources):
    from spark_tfrecord_amd.engine import gpu as gpu_engine
    return [gpu_engine.batch_to_device(s) for s in sources]


@pytest.mark.parametrize("name", C.case_names())
def test_kernel_matches_host_core(name):
    case = C.case(name)
    want, want_status = collate_batch(case.sources, case.sel_slot,
                                      case.sel_row, case.specs, "cpu",
                                      return_status=True)
    dev = to_device(case.sources)
    got, status = collate_batch(dev, case.sel_slot, case.sel_row, case.specs,
                                "gpu", return_status=True)
    assert all(t.is_cuda for t in got.values())
    assert status == want_status
    # outputs are defined on an error too (the cut or filled cell), and the
    # two runs of one core agree on them
    assert_same(got, want)
    if case.expect_error is not None:
        b, c, cause = case.expect_error
        assert status[0] == (b << 16) | (c << 8) | cause
        with pytest.raises(ValueError, match=f"batch row {b}"):
            collate_batch(dev, case.sel_slot, case.sel_row, case.specs, "gpu")
    else:
        assert status == (STATUS_CLEAN, case.expect_truncated)
        assert_same(got, case.expect)


def test_one_window_many_batches_and_preallocated_outputs():
    """The dataset's use: one uploaded window, several selections; outputs
    the caller owns are filled in place, padding included."""
    case = C.case("column-table")
    co = Collator(case.sources[0].schema, case.specs, "gpu")
    co.set_window(to_device(case.sources))
    out = {k: torch.full(v.shape, 77, dtype=torch.from_numpy(v).dtype,
                         device="cuda") for k, v in case.expect.items()}
    got, status = co.run(case.sel_slot, case.sel_row, out)
    assert all(got[k] is out[k] for k in out)
    assert status == (STATUS_CLEAN, case.expect_truncated)
    assert_same(out, case.expect)
    rev = slice(None, None, -1)
    got, _ = co.run(case.sel_slot[rev], case.sel_row[rev])
    assert_same(got, {k: v[rev] for k, v in case.expect.items()})
    assert co.launches == 2 and co.host_waits == 2


# ---------------------------------------------------------------------------
# datasets: engine="gpu" == engine="cpu"
# ---------------------------------------------------------------------------

ROWS = 2500
FEATURES = {"uid": FixedLen(), "vec": FixedLen(5),
            "ints": Padded(3, pad=-1, truncate=True),
            "opt": FixedLen(default=-4.5),
            "tags": Padded2D(2, 5, pad=0x20, truncate=True)}


def _data():
    rng = np.random.default_rng(3)
    return {
        "uid": np.arange(ROWS, dtype=np.int64),
        "vec": [rng.random(5).astype(np.float32).tolist()
                for _ in range(ROWS)],
        "ints": [[i * 10 + k for k in range(i % 5)] for i in range(ROWS)],
        "opt": [None if i % 4 == 0 else float(i) / 8 for i in range(ROWS)],
        "tags": [[f"tag{i % 11}x"[: 3 + i % 4]] * (i % 4)
                 for i in range(ROWS)],
    }


@pytest.fixture(scope="module")
def cpu_written(tmp_path_factory):
    root = tmp_path_factory.mktemp("collate_gpu")
    data = _data()
    outs = {}
    for codec in (None, "gzip", "snappy"):
        out = str(root / f"ds_{codec}")
        stf.write_tfrecord(data, out, engine="cpu", num_shards=5, codec=codec)
        outs[codec] = out
    return outs, data


def _pair(out, **kw):
    cpu = TFRecordBatchDataset(out, FEATURES, engine="cpu", batch_size=300,
                               shuffle_window=3, seed=11, **kw)
    gpu = TFRecordBatchDataset(out, FEATURES, engine="gpu", batch_size=300,
                               shuffle_window=3, seed=11, schema=cpu.schema,
                               **kw)
    return cpu, gpu


@pytest.mark.parametrize("codec", [None, "gzip", "snappy"])
def test_dataset_gpu_equals_cpu(cpu_written, codec):
    outs, data = cpu_written
    cpu, gpu = _pair(outs[codec])
    a, b = list(cpu), list(gpu)
    assert len(a) == len(b) == (ROWS + 299) // 300
    uids = []
    for x, y in zip(a, b):
        assert all(t.is_cuda for t in y.values())
        assert not any(t.is_cuda for t in x.values())
        assert_same(y, x)
        uids.append(x["uid"].numpy())
    assert sorted(np.concatenate(uids).tolist()) == list(range(ROWS))
    want = sum(1 for i in range(ROWS) if i % 5 > 3 or i % 4 > 2)
    assert cpu.truncated_rows == gpu.truncated_rows == want
    # one launch and one host wait per batch
    assert gpu.last_stats == {"batches": len(b), "launches": len(b),
                              "host_waits": len(b)}
    # the values are the written ones
    u = int(a[0]["uid"][0])
    assert float(a[0]["opt"][0]) == (-4.5 if u % 4 == 0 else u / 8)
    assert a[0]["ints"][0].tolist() == \
        (data["ints"][u] + [-1] * 3)[:3]


def test_dataset_gpu_no_shuffle_and_epochs(cpu_written):
    outs, _ = cpu_written
    cpu = TFRecordBatchDataset(outs[None], FEATURES, engine="cpu",
                               batch_size=999, shuffle_window=0)
    gpu = TFRecordBatchDataset(outs[None], FEATURES, engine="gpu",
                               batch_size=999, shuffle_window=0,
                               schema=cpu.schema, prefetch=0)
    for x, y in zip(list(cpu), list(gpu)):
        assert_same(y, x)
    cpu, gpu = _pair(outs[None])
    cpu.set_epoch(2)
    gpu.set_epoch(2)
    for x, y in zip(list(cpu), list(gpu)):
        assert_same(y, x)


def test_dataset_gpu_error_names_shard_and_row(cpu_written):
    outs, _ = cpu_written
    specs = {"uid": FixedLen(), "ints": Padded(3)}
    cpu = TFRecordBatchDataset(outs[None], specs, engine="cpu",
                               batch_size=300, shuffle_window=2, seed=1)
    gpu = TFRecordBatchDataset(outs[None], specs, engine="gpu",
                               batch_size=300, shuffle_window=2, seed=1,
                               schema=cpu.schema)
    with pytest.raises(ValueError) as ec:
        list(cpu)
    with pytest.raises(ValueError) as eg:
        list(gpu)
    assert str(eg.value) == str(ec.value)
    assert "'ints'" in str(eg.value) and "shard " in str(eg.value)


def test_sequence_example_feature_list(tmp_path):
    out = str(tmp_path / "seq")
    rows = 700
    schema = stf.StructType([
        stf.StructField("uid", stf.LongType(), True),
        stf.StructField("steps", stf.ArrayType(stf.ArrayType(stf.LongType())),
                        True),
        stf.StructField("obs", stf.ArrayType(stf.ArrayType(stf.FloatType())),
                        True),
    ])
    data = {
        "uid": list(range(rows)),
        "steps": [[[i, k, j] [: 1 + (j % 3)] for j in range(k)]
                  for i in range(rows) for k in [i % 4]],
        "obs": [[[float(i) + 0.5] * (j + 1) for j in range(i % 3)]
                for i in range(rows)],
    }
    stf.write_tfrecord(data, out, engine="cpu", num_shards=3, schema=schema,
                       record_type="SequenceExample")
    specs = {"uid": FixedLen(), "steps": Padded2D(3, 3, pad=-1),
             "obs": Padded2D(2, 2, truncate=True)}
    kw = dict(record_type="SequenceExample", schema=schema, batch_size=256,
              shuffle_window=2, seed=4)
    a = list(TFRecordBatchDataset(out, specs, engine="cpu", **kw))
    b = list(TFRecordBatchDataset(out, specs, engine="gpu", **kw))
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert y["steps"].is_cuda and y["steps"].shape[1:] == (3, 3)
        assert_same(y, x)
    u = int(a[0]["uid"][1])
    k = u % 4
    assert int(a[0]["steps_outer"][1]) == k
    assert a[0]["steps_len"][1].tolist() == \
        [1 + (j % 3) if j < k else 0 for j in range(3)]
