"""CPU tier of the batch collation: the host run of csrc/collate_core.h
against the Python reference of collate_cases.py, the spec/schema pairing
and geometry checks, and TFRecordBatchDataset(engine="cpu")."""

import numpy as np
import pytest
import torch

import spark_tfrecord_amd as stf
from spark_tfrecord_amd import collate as CL
from spark_tfrecord_amd.collate import (STATUS_CLEAN, FixedLen, Padded,
                                        Padded2D, collate_batch)
from spark_tfrecord_amd.torch_data import TFRecordBatchDataset

import collate_cases as C


def bits(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_outputs_equal(got: dict, want: dict):
    assert set(got) == set(want)
    for k in want:
        g, w = bits(got[k]), bits(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert np.array_equal(g, w), k


# ---------------------------------------------------------------------------
# host core == reference
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.case_names())
def test_host_collate_matches_reference(name):
    case = C.case(name)
    outs, (st0, trunc) = collate_batch(case.sources, case.sel_slot,
                                       case.sel_row, case.specs, "cpu",
                                       return_status=True)
    if case.expect_error is not None:
        b, c, cause = case.expect_error
        assert st0 == (b << 16) | (c << 8) | cause
        with pytest.raises(ValueError) as e:
            collate_batch(case.sources, case.sel_slot, case.sel_row,
                          case.specs, "cpu")
        assert f"'{list(case.specs)[c]}'" in str(e.value)
        assert ("MISSING" if cause == C.MISSING else "LENGTH") in str(e.value)
        assert f"batch row {b}" in str(e.value)
        return
    assert st0 == STATUS_CLEAN
    assert trunc == case.expect_truncated
    assert_outputs_equal(outs, case.expect)


def test_cases_cover_what_they_claim():
    cases = C.all_cases()
    assert any(c.expect_truncated for c in cases)
    assert sum(c.expect_error is not None for c in cases) >= 9
    table = C.case("column-table")
    assert table.sources[1].num_rows == 0
    assert set(table.sel_slot.tolist()) == {0, 2, 3}
    assert table.expect_truncated > 0
    # negative zero and a NaN payload went through some float column
    seen = set()
    for c in cases:
        for k, v in (c.expect or {}).items():
            if v.dtype == np.float32:
                seen |= set(np.unique(v.view(np.uint32)).tolist()) & set(
                    C.FLOAT_ODDITIES)
    assert {0x80000000, 0x7FC12345} <= seen


# ---------------------------------------------------------------------------
# spec / schema pairing
# ---------------------------------------------------------------------------

def _schema():
    return stf.StructType([
        stf.StructField("i", stf.LongType(), True),
        stf.StructField("fs", stf.ArrayType(stf.FloatType()), True),
        stf.StructField("s", stf.StringType(), True),
        stf.StructField("ss", stf.ArrayType(stf.StringType()), True),
        stf.StructField("fl", stf.ArrayType(stf.ArrayType(stf.LongType())),
                        True),
        stf.StructField("fls", stf.ArrayType(stf.ArrayType(stf.StringType())),
                        True),
        stf.StructField("nul", stf.NullType(), True),
    ])


@pytest.mark.parametrize("name,spec", [
    ("fls", Padded2D(2, 2)),      # FeatureList of bytes: three levels
    ("s", FixedLen()),            # numeric spec on a bytes column
    ("ss", Padded(4)),
    ("fl", Padded(4)),            # one-level spec on a FeatureList
    ("fl", FixedLen(2)),
    ("i", Padded2D(1, 1)),        # two-level spec on a flat numeric column
    ("fs", Padded2D(1, 4)),
    ("nul", FixedLen()),          # NullType
    ("nope", FixedLen()),         # not in the schema
    ("i", "FixedLen"),            # not a spec
    ("fs", Padded(0)),
    ("fs", FixedLen(-1)),
])
def test_bad_pairing_names_the_column(name, spec):
    with pytest.raises(ValueError) as e:
        CL.plan_columns(_schema(), {name: spec})
    assert f"'{name}'" in str(e.value)


def test_good_pairings_and_column_limit():
    plans = CL.plan_columns(_schema(), {
        "i": FixedLen(), "fs": Padded(3, pad=1.5), "s": Padded2D(1, 8),
        "ss": Padded2D(2, 8), "fl": Padded2D(2, 2)})
    assert [p.mode for p in plans] == [0, 1, 2, 2, 2]
    many = stf.StructType([stf.StructField(f"c{i}", stf.LongType(), True)
                           for i in range(65)])
    with pytest.raises(ValueError, match="at most 64"):
        CL.plan_columns(many, {f"c{i}": FixedLen() for i in range(65)})
    CL.plan_columns(many, {f"c{i}": FixedLen() for i in range(64)})


def test_dataset_checks_pairing_at_construction(tmp_sandbox):
    out = str(tmp_sandbox / "ds")
    stf.write_tfrecord({"x": np.arange(10, dtype=np.int64)}, out, engine="cpu")
    with pytest.raises(ValueError, match="'x'"):
        TFRecordBatchDataset(out, {"x": Padded2D(1, 1)}, engine="cpu")
    with pytest.raises(ValueError, match="'y'"):
        TFRecordBatchDataset(out, {"y": FixedLen()}, engine="cpu")


# ---------------------------------------------------------------------------
# geometry: refused before any native call
# ---------------------------------------------------------------------------

@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("native collation reached")
    monkeypatch.setattr(CL._native, "host_collate", boom)
    monkeypatch.setattr(CL._native, "gpu_collate_rows", boom)


def test_geometry_is_checked_first(no_native):
    case = C.case("column-table")
    n = len(case.sources)
    B = len(case.sel_slot)

    def run(slot, row, out=None):
        return collate_batch(case.sources, slot, row, case.specs, "cpu",
                             out=out)

    slot = case.sel_slot.copy()
    slot[3] = n
    with pytest.raises(ValueError, match="batch row 3: slot"):
        run(slot, case.sel_row)
    slot[3] = -1
    with pytest.raises(ValueError, match="batch row 3: slot"):
        run(slot, case.sel_row)
    row = case.sel_row.copy()
    row[7] = case.sources[case.sel_slot[7]].num_rows
    with pytest.raises(ValueError, match="batch row 7: row"):
        run(case.sel_slot, row)
    row[7] = -1
    with pytest.raises(ValueError, match="batch row 7: row"):
        run(case.sel_slot, row)
    slot = case.sel_slot.copy()
    slot[0] = 1  # the empty slot has no row 0
    with pytest.raises(ValueError, match="batch row 0: row"):
        run(slot, case.sel_row)
    with pytest.raises(ValueError):
        run(case.sel_slot[:-1], case.sel_row)
    with pytest.raises(ValueError):
        run(case.sel_slot[:0], case.sel_row[:0])

    good = {k: torch.empty(v.shape, dtype=torch.from_numpy(v).dtype)
            for k, v in case.expect.items()}
    for key, bad in [
        ("tokens", torch.empty((B, 2, 13), dtype=torch.uint8)),
        ("tokens", torch.empty((B + 1, 2, 12), dtype=torch.uint8)),
        ("ints", torch.empty((B, 8), dtype=torch.int32)),
        ("ints_len", torch.empty((B, 1), dtype=torch.int32)),
        ("big", torch.empty((B, 65, 5), dtype=torch.float32).transpose(1, 2)),
    ]:
        with pytest.raises(ValueError, match=key):
            run(case.sel_slot, case.sel_row, dict(good, **{key: bad}))
    with pytest.raises(ValueError, match="expected tensors"):
        run(case.sel_slot, case.sel_row,
            {k: v for k, v in good.items() if k != "id"})
    # and a well-formed call does reach it
    with pytest.raises(AssertionError, match="native collation reached"):
        run(case.sel_slot, case.sel_row, good)


def test_preallocated_outputs_are_filled():
    case = C.case("column-table")
    out = {k: torch.full(v.shape, 99, dtype=torch.from_numpy(v).dtype)
           for k, v in case.expect.items()}
    got = collate_batch(case.sources, case.sel_slot, case.sel_row, case.specs,
                        "cpu", out=out)
    assert all(got[k] is out[k] for k in out)
    assert_outputs_equal(out, case.expect)


# ---------------------------------------------------------------------------
# TFRecordBatchDataset, CPU engine
# ---------------------------------------------------------------------------

ROWS, SHARDS = 3001, 4
FEATURES = {"uid": FixedLen(), "score": FixedLen(1),
            "ints": Padded(3, pad=-1), "tags": Padded2D(2, 4, pad=0x20)}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("collate") / "ds")
    rng = np.random.default_rng(0)
    data = {
        "uid": np.arange(ROWS, dtype=np.int64),
        "score": rng.random(ROWS).astype(np.float32),
        "ints": [[i + k for k in range(i % 4)] for i in range(ROWS)],
        "tags": [[f"t{i % 7}"] * (i % 3) for i in range(ROWS)],
    }
    stf.write_tfrecord(data, out, engine="cpu", num_shards=SHARDS)
    return out, data


def _ds(out, **kw):
    kw.setdefault("engine", "cpu")
    kw.setdefault("batch_size", 700)
    return TFRecordBatchDataset(out, FEATURES, **kw)


def _ids(ds):
    return [b["uid"].numpy().copy() for b in ds]


def _read_uids(path):
    ds = TFRecordBatchDataset(path, {"uid": FixedLen()}, batch_size=1 << 20,
                              shuffle_window=0, engine="cpu")
    return np.concatenate(_ids(ds)).tolist()


def test_batch_sizes_and_drop_last(dataset):
    out, _ = dataset
    for window in (0, 1, 3):
        sizes = [len(x) for x in _ids(_ds(out, shuffle_window=window))]
        assert sizes == [700] * 4 + [ROWS - 2800]
        sizes = [len(x) for x in _ids(_ds(out, shuffle_window=window,
                                          drop_last=True))]
        assert sizes == [700] * 4
    # a batch larger than any shard still fills up, across several shards
    sizes = [len(x) for x in _ids(_ds(out, shuffle_window=1,
                                      batch_size=2000))]
    assert sizes == [2000, ROWS - 2000]


def test_no_shuffle_is_file_order(dataset):
    out, _ = dataset
    ids = np.concatenate(_ids(_ds(out, shuffle_window=0)))
    file_order = []
    from spark_tfrecord_amd.io import paths as P
    for p in P.list_data_files(out):
        file_order += _read_uids(p)
    assert ids.tolist() == file_order
    assert sorted(file_order) == list(range(ROWS))


@pytest.mark.parametrize("window", [1, 3])
def test_shuffle_is_a_seeded_permutation(dataset, window):
    out, _ = dataset
    ds = _ds(out, shuffle_window=window, seed=5)
    e0 = np.concatenate(_ids(ds))
    assert sorted(e0.tolist()) == list(range(ROWS))
    assert e0.tolist() != sorted(e0.tolist())
    again = np.concatenate(_ids(_ds(out, shuffle_window=window, seed=5)))
    assert np.array_equal(e0, again)
    ds.set_epoch(1)
    e1 = np.concatenate(_ids(ds))
    assert sorted(e1.tolist()) == list(range(ROWS))
    assert not np.array_equal(e0, e1)
    ds.set_epoch(0)
    assert np.array_equal(e0, np.concatenate(_ids(ds)))
    other = np.concatenate(_ids(_ds(out, shuffle_window=window, seed=6)))
    assert not np.array_equal(e0, other)


def test_window_bounds_the_shards_of_a_batch(dataset):
    out, _ = dataset
    from spark_tfrecord_amd.io import paths as P
    where = {}
    for k, p in enumerate(P.list_data_files(out)):
        for u in _read_uids(p):
            where[u] = k
    for batch in _ids(_ds(out, shuffle_window=1)):
        shards = sorted({where[int(u)] for u in batch})
        assert len(shards) <= 2
        assert shards[-1] - shards[0] <= 1
    first = _ids(_ds(out, shuffle_window=3))[0]
    assert len({where[int(u)] for u in first}) > 1


def test_dense_outputs_match_the_written_data(dataset):
    out, data = dataset
    for window in (0, 3):
        seen = 0
        for b in _ds(out, shuffle_window=window):
            uid = b["uid"].numpy()
            assert b["score"].shape == (len(uid), 1)
            assert b["ints"].dtype == torch.int64
            assert b["tags"].dtype == torch.uint8
            assert b["tags"].shape == (len(uid), 2, 4)
            assert np.array_equal(b["score"].numpy()[:, 0].view(np.int32),
                                  data["score"][uid].view(np.int32))
            for k, u in enumerate(uid.tolist()):
                want = data["ints"][u]
                n = len(want)
                assert int(b["ints_len"][k]) == n
                assert b["ints"][k].tolist() == want + [-1] * (3 - n)
                tags = data["tags"][u]
                assert int(b["tags_outer"][k]) == len(tags)
                assert b["tags_len"][k].tolist() == \
                    [len(t) for t in tags] + [0] * (2 - len(tags))
                raw = bytes(b["tags"][k].numpy().tobytes())
                assert raw == b"".join(t.encode().ljust(4) for t in tags) \
                    + b" " * (4 * (2 - len(tags)))
            seen += len(uid)
        assert seen == ROWS


def test_error_names_shard_and_row(dataset):
    out, data = dataset
    from spark_tfrecord_amd.io import paths as P
    ds = TFRecordBatchDataset(out, {"uid": FixedLen(), "ints": Padded(2)},
                              batch_size=700, shuffle_window=0, engine="cpu")
    with pytest.raises(ValueError) as e:
        list(ds)
    # file order: the first row with three values is the first bad one
    files = P.list_data_files(out)
    first = _read_uids(files[0])
    row = next(k for k, u in enumerate(first) if len(data["ints"][u]) == 3)
    msg = str(e.value)
    assert "'ints'" in msg and "LENGTH" in msg
    assert f"shard {files[0]}" in msg
    assert msg.endswith(f"row {row}")


def test_truncated_rows_accumulate(dataset):
    out, data = dataset
    ds = TFRecordBatchDataset(
        out, {"ints": Padded(2, truncate=True),
              "tags": Padded2D(1, 1, truncate=True)},
        batch_size=512, shuffle_window=2, engine="cpu")
    n = sum(b["ints"].shape[0] for b in ds)
    assert n == ROWS
    want = sum(1 for i in range(ROWS)
               if len(data["ints"][i]) > 2 or len(data["tags"][i]) > 0)
    assert ds.truncated_rows == want
    assert ds.last_stats["batches"] == (ROWS + 511) // 512


def test_prefetch_depth_does_not_change_batches(dataset):
    out, _ = dataset
    a = list(_ds(out, shuffle_window=3, prefetch=0, seed=2))
    b = list(_ds(out, shuffle_window=3, prefetch=2, seed=2))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert_outputs_equal(x, y)
