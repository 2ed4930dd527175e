"""Padded3D / Ragged3D batches of a bytes FeatureList, CPU engine, exact
against numpy loops over the Python lists the files were written from. The
rows, `reference_*` and the check bodies are shared with
test_gpu_collate3d.py."""

import functools
import tempfile

import numpy as np
import pytest

import spark_tfrecord_amd as stf
from spark_tfrecord_amd.collate import (STATUS_CLEAN, FixedLen, Padded,
                                        Padded2D, Padded3D, Ragged3D,
                                        collate_batch, plan_columns)
from spark_tfrecord_amd.engine import cpu as cpu_engine
from spark_tfrecord_amd.io import paths as P
from spark_tfrecord_amd.torch_data import TFRecordBatchDataset

LENGTH, CAPACITY = 2, 4
SCHEMA = stf.StructType([
    stf.StructField("uid", stf.LongType(), True),
    stf.StructField("toks", stf.ArrayType(stf.LongType()), True),
    stf.StructField("f", stf.ArrayType(stf.ArrayType(stf.BinaryType())), True),
    stf.StructField("g", stf.ArrayType(stf.ArrayType(stf.BinaryType())), True),
])
# (B, S, T, L); the cell table holds tiles of up to 1024 cells, which every
# tile is from L = 8 on: (130, 3, 3, 7) is one tile of 1170 cells (the per-unit
# walk), (97, 3, 3, 13) two tiles of 631 and 243 (the table)
SHAPES = [(5, 2, 2, 5), (97, 3, 3, 13), (9, 4, 1, 1024), (130, 3, 3, 7)]


def _rows(S, T, L, seed):
    """One slot: the special rows, then random ones."""
    rng = np.random.default_rng(seed)

    def s(n):
        return bytes(rng.integers(1, 256, n, dtype=np.uint8).tolist())

    def step():
        return [s(int(rng.choice([0, 1, L, L + 3, rng.integers(0, L + 1)])))
                for _ in range(int(rng.integers(0, T + 2)))]

    rows = [None, [], [[]], [[b""], [s(1), s(7)]], [[s(8)], [s(9)]],
            [[s(L + 3)]], [[s(2)] for _ in range(S + 1)],
            [[s(3) for _ in range(T + 1)]]]
    rows += [[step() for _ in range(int(rng.integers(0, S + 2)))]
             for _ in range(16)]
    return rows[::-1] if seed % 2 else rows


@functools.lru_cache(maxsize=None)
def window(S, T, L):
    """Two slots written as SequenceExample files by the CPU engine and
    decoded again -> (rows per slot, decoded RecordBatches)."""
    rows, sources = [], []
    for slot in range(2):
        f = _rows(S, T, L, 10 * L + slot)
        data = {"uid": list(range(len(f))),
                "toks": [[k] * (k % 6) for k in range(len(f))],
                "f": f, "g": f[::-1]}
        with tempfile.TemporaryDirectory() as d:
            stf.write_tfrecord(data, d + "/w", record_type="SequenceExample",
                               schema=SCHEMA, engine="cpu")
            blob = b"".join(P.decompress_file(p)
                            for p in P.list_data_files(d + "/w"))
        sources.append(cpu_engine.decode_buffer(
            np.frombuffer(blob, np.uint8), SCHEMA, "SequenceExample", True))
        rows.append(f)
    return rows, sources


def selection(B, rows):
    slot = np.arange(B, dtype=np.int32) % 2
    # a stride coprime with the 24 rows: small batches reach special rows
    row = np.array([5 * (b // 2) % len(rows[s]) for b, s in enumerate(slot)],
                   np.int64)
    return slot, row, [rows[s][r] or [] for s, r in zip(slot, row)]


def reference_padded(picked, S, T, L, pad, truncate):
    B = len(picked)
    out = {"f": np.full((B, S, T, L), pad, np.uint8),
           "f_steps": np.zeros(B, np.int32),
           "f_outer": np.zeros((B, S), np.int32),
           "f_len": np.zeros((B, S, T), np.int32)}
    over = np.zeros(B, bool)
    for b, row in enumerate(picked):
        over[b] = len(row) > S
        out["f_steps"][b] = min(len(row), S)
        for s, step in enumerate(row[:S]):
            over[b] |= len(step) > T
            out["f_outer"][b, s] = min(len(step), T)
            for t, x in enumerate(step[:T]):
                over[b] |= len(x) > L
                n = out["f_len"][b, s, t] = min(len(x), L)
                out["f"][b, s, t, :n] = np.frombuffer(x[:n], np.uint8)
    if truncate or not over.any():
        return out, STATUS_CLEAN, int(over.sum())
    return out, (int(np.argmax(over)) << 16) | LENGTH, 0


def reference_ragged(picked, scap, icap, cap):
    steps = [st for row in picked for st in row]
    strings = [x for st in steps for x in st]
    flat = np.frombuffer(b"".join(strings), np.uint8)
    ends = []  # per level: every row's raw end
    for count in (len, lambda r: sum(map(len, r)),
                  lambda r: sum(len(x) for st in r for x in st)):
        ends.append(np.cumsum([0] + [count(r) for r in picked]))

    def offsets(lens, n, clamp):  # n+1 entries, the total repeated
        cum = np.cumsum([0] + lens)
        cum = np.concatenate([cum, np.full(n + 1, cum[-1])])[:n + 1]
        return np.minimum(cum, clamp).astype(np.int32)

    out = {"f": np.concatenate([flat, np.zeros(cap, np.uint8)])[:cap],
           "f_item_offsets": offsets([len(x) for x in strings], icap, cap),
           "f_step_offsets": offsets([len(st) for st in steps], scap, icap),
           "f_offsets": np.minimum(ends[0], scap).astype(np.int32)}
    over = ((ends[0] > scap) | (ends[1] > icap) | (ends[2] > cap))[1:]
    st0 = (int(np.argmax(over)) << 16) | CAPACITY if over.any() else STATUS_CLEAN
    return out, st0, 0, [int(e[-1]) for e in ends]


def check(engine, sources, slot, row, spec, want):
    got, status = collate_batch(sources, slot, row, {"f": spec}, engine,
                                return_status=True)
    assert status == (want[1], want[2])
    assert set(got) == set(want[0])
    for k, w in want[0].items():
        g = got[k].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert np.array_equal(g, w), k


def padded_case(engine, shape, truncate, to_device=lambda s: s):
    B, S, T, L = shape
    rows, sources = window(S, T, L)
    slot, row, picked = selection(B, rows)
    want = reference_padded(picked, S, T, L, 0x2E, truncate)
    assert (want[2] > 0) if truncate else (want[1] != STATUS_CLEAN)
    check(engine, to_device(sources), slot, row,
          Padded3D(S, T, L, pad=0x2E, truncate=truncate), want)


def ragged_case(engine, short, to_device=lambda s: s):
    """short: None, or the level (0 steps, 1 items, 2 values) whose capacity
    is one below the batch's total."""
    rows, sources = window(3, 3, 13)
    slot, row, picked = selection(97, rows)
    totals = reference_ragged(picked, 1, 1, 1)[3]
    caps = [n + 5 - (6 if k == short else 0) for k, n in enumerate(totals)]
    want = reference_ragged(picked, *caps)
    assert (want[1] == STATUS_CLEAN) == (short is None)
    check(engine, to_device(sources), slot, row, Ragged3D(*caps), want)


def dataset_case(tmp_path, engines):
    """-> per engine, (dataset, batches); the data's rows by uid."""
    f, g = _rows(3, 2, 9, 4) * 9, _rows(2, 2, 6, 6) * 9
    data = {"uid": list(range(len(f))),
            "toks": [[k] * (k % 6) for k in range(len(f))], "f": f, "g": g}
    out = str(tmp_path / "ds")
    stf.write_tfrecord(data, out, record_type="SequenceExample", schema=SCHEMA,
                       engine="cpu", num_shards=3)
    feats = {"uid": FixedLen(), "toks": Padded(4, truncate=True),
             "f": Padded3D(3, 2, 9, truncate=True),
             "g": Ragged3D(400, 800, 4000)}
    res = []
    for eng in engines:
        ds = TFRecordBatchDataset(out, feats, engine=eng, schema=SCHEMA,
                                  record_type="SequenceExample", batch_size=64,
                                  shuffle_window=2, seed=3)
        res.append((ds, list(ds)))
    return res, data


@pytest.mark.parametrize("shape", SHAPES)
def test_padded3d_truncating(shape):
    padded_case("cpu", shape, True)


def test_padded3d_length_error():
    padded_case("cpu", SHAPES[1], False)


@pytest.mark.parametrize("short", [None, 0, 1, 2])
def test_ragged3d(short):
    ragged_case("cpu", short)


def test_dataset_yields_the_written_rows(tmp_path):
    [(ds, batches)], data = dataset_case(tmp_path, ["cpu"])
    assert len(batches) == 4 and ds.truncated_rows > 0
    for x in batches:
        picked_f = [data["f"][u] or [] for u in x["uid"].tolist()]
        picked_g = [data["g"][u] or [] for u in x["uid"].tolist()]
        want = reference_padded(picked_f, 3, 2, 9, 0, True)[0]
        want.update({"g" + k[1:]: v for k, v in
                     reference_ragged(picked_g, 400, 800, 4000)[0].items()})
        for k, w in want.items():
            assert np.array_equal(x[k].numpy(), w), k


def test_plan_errors():
    for name, spec in (("toks", Padded3D(2, 2, 2)), ("uid", Ragged3D(4, 4, 4)),
                       ("f", Padded2D(2, 2)), ("f", Padded3D(2, 0, 2)),
                       ("f", Ragged3D(4, -1, 4)),
                       ("f", Padded3D(2, 2, 2, dtype="int32"))):
        with pytest.raises(ValueError, match=f"'{name}'"):
            plan_columns(SCHEMA, {name: spec})
