"""Packed (Ragged / Ragged2D) and int32 batch outputs, CPU engine, bit-exact
against a numpy reference built from the Python lists the sources were made
from. The cases and `check` are shared with test_gpu_collate_ragged.py."""

import functools

import numpy as np
import pytest

from spark_tfrecord_amd.collate import (STATUS_CLEAN, FixedLen, Padded,
                                        Padded2D, Ragged, Ragged2D,
                                        collate_batch, plan_columns)
from spark_tfrecord_amd.columnar import RecordBatch

import collate_cases as C

RANGE, CAPACITY = 3, 4
LO, HI = -2**31, 2**31 - 1
I1, F1, I2, F2, S2 = C.I1, C.F1, C.I2, C.F2, C.S2
_DT = {"i": np.int64, "f": np.uint32, "s": np.uint8}


def make(cols, rows, specs, slot, row):
    schema = C.schema_of(cols)
    sources = [RecordBatch(schema, [C.wire_column(sh, sl[n]) for n, sh in cols],
                           len(sl[cols[0][0]])) for sl in rows]
    return dict(cols=dict(cols), rows=rows, specs=specs, sources=sources,
                slot=np.asarray(slot, np.int32), row=np.asarray(row, np.int64))


def reference(case):
    """-> (outputs, status word, truncated rows)"""
    B = len(case["slot"])
    out, errs, cut = {}, [], np.zeros(B, bool)
    for c, (name, spec) in enumerate(case["specs"].items()):
        shape = case["cols"][name]
        rows = [case["rows"][s][name][r]
                for s, r in zip(case["slot"], case["row"])]
        if not isinstance(spec, (Ragged, Ragged2D)):
            cells = [C.reference_cell(shape, spec, r) for r in rows]
            cut |= [tr for _, tr, _ in cells]
            for k in cells[0][0]:
                out[name + k] = np.array([o[k] for o, _, _ in cells],
                                         np.int32 if k else _DT[shape[0]])
            vals = out[name].reshape(B, -1)
            if isinstance(spec, FixedLen) and spec.length is None:
                out[name] = out[name].reshape(B)
            voff = np.arange(B + 1) * vals.shape[1]
        else:
            two = isinstance(spec, Ragged2D)
            groups = [list(r or []) for r in rows]  # values, or items
            if not two and spec.max_len:
                cut |= [len(g) > spec.max_len for g in groups]
                groups = [g[:spec.max_len] for g in groups]
            cap = spec.value_capacity if two else (spec.capacity
                                                   or B * spec.max_len)
            off, over = np.cumsum([0] + [len(g) for g in groups]), False
            if two:  # row -> items -> values: offsets over items, then flatten
                icap = spec.item_capacity
                cum = np.cumsum([0] + [len(x) for r in groups for x in r])
                io = np.concatenate([cum, np.full(icap + 1, cum[-1])])
                out[name + "_item_offsets"] = np.minimum(
                    io[:icap + 1], cap).astype(np.int32)
                out[name + "_offsets"] = np.minimum(off, icap).astype(np.int32)
                over = off[1:] > icap
                groups = [[v for x in r for v in x] for r in groups]
            voff = np.cumsum([0] + [len(g) for g in groups])
            flat = np.array([v for g in groups for v in g], _DT[shape[0]])
            vals = np.concatenate([flat, np.zeros(cap, flat.dtype)])[:cap]
            over = over | (voff[1:] > cap)
            if over.any():
                errs.append((int(np.argmax(over)), c, CAPACITY))
            if not two:
                out[name + "_offsets"] = np.minimum(voff, cap).astype(np.int32)
            out[name] = vals
        if spec.dtype:
            bad = np.flatnonzero(vals.reshape(-1) != vals.reshape(-1).astype(
                np.int32))
            if len(bad):
                b = int(np.searchsorted(voff, bad[0], "right")) - 1
                errs.append((b, c, RANGE))
            out[name] = out[name].astype(np.int32)  # the low 32 bits
    st0 = min(((b << 16) | (c << 8) | e for b, c, e in errs),
              default=STATUS_CLEAN)
    return out, st0, int(cut.sum())


def check(case, engine, sources=None):
    got, (st0, trunc) = collate_batch(
        sources or case["sources"], case["slot"], case["row"], case["specs"],
        engine, return_status=True)
    want, want_st0, want_trunc = reference(case)
    assert (st0, trunc) == (want_st0, want_trunc)
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k].cpu().numpy()
        g = g.view(np.uint32) if g.dtype == np.float32 else g
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert np.array_equal(g, w), k
    return want_st0


def _rows(rng, shape, R, max_items=3, max_len=5):
    """Absent rows, then 0..max_len values, or 0..max_items items of them."""
    def one():
        return C._vals(rng, shape[0], int(rng.integers(0, max_len + 1)))
    return [None if rng.random() < 0.15 else one() if shape[1] == 1
            else [one() for _ in range(int(rng.integers(0, max_items + 1)))]
            for _ in range(R)]


COLS = [("a", I1), ("f", F1), ("s", S2), ("l", I2), ("g", F2)]


def _scan(B, slack=(3, 2, 5, 1, 3)):
    """Two slots, shuffled with repeats; slack[i]: capacity i minus the total."""
    rng = np.random.default_rng(B)
    slot_rows = [7, 40]
    rows = [{n: _rows(rng, sh, R) for n, sh in COLS} for R in slot_rows]
    slot, row = C._selection(rng, B, slot_rows)
    pick = {n: [rows[s][n][r] or [] for s, r in zip(slot, row)]
            for n, _ in COLS}
    vals = {n: sum(len(r) if sh[1] == 1 else sum(map(len, r)) for r in pick[n])
            for n, sh in COLS}
    items = {n: sum(map(len, pick[n])) for n in "slg"}
    specs = {"a": Ragged(capacity=max(vals["a"] + slack[0], 1)),
             "f": Ragged(max_len=3),
             "s": Ragged2D(max(items["s"] + slack[1], 1),
                           max(vals["s"] + slack[2], 1)),
             "l": Ragged2D(max(items["l"] + slack[3], 1),
                           max(vals["l"] + slack[4], 1)),
             "g": Ragged2D(items["g"] + 2000, vals["g"] + 1027)}
    return make(COLS, rows, specs, slot, row)


def _gather(lens):
    """One slot in file order; row k has lens[k] values."""
    rng = np.random.default_rng(len(lens))
    cols = [("a", I1), ("f", F1), ("s", S2)]
    rows = [{"a": [C._vals(rng, "i", n) for n in lens],
             "f": [C._vals(rng, "f", n) if n else None for n in lens],
             "s": [[C._vals(rng, "s", n)] if n else [] for n in lens]}]
    specs = dict(a=Ragged(4099), f=Ragged(4099), s=Ragged2D(11, 4099))
    return make(cols, rows, specs, np.zeros(len(lens)), np.arange(len(lens)))


def _bytes():
    """Strings of 0..17 bytes, 0..3 per row: every (source, output) start
    misalignment of a row that holds a whole output word."""
    rng = np.random.default_rng(8)
    slot_rows, B = [150, 90], 1200
    rows = [{"s": _rows(rng, S2, R, 3, 17)} for R in slot_rows]
    slot, row = C._selection(rng, B, slot_rows)
    start = [np.cumsum([1] + [sum(map(len, r or [])) for r in sl["s"]])
             for sl in rows]
    n = np.array([sum(map(len, rows[s]["s"][r] or []))
                  for s, r in zip(slot, row)])
    out = np.cumsum(n) - n
    pairs = {(start[s][r] % 8, o % 8)
             for s, r, o, k in zip(slot, row, out, n) if k >= 15}
    assert len(pairs) == 64
    return make([("s", S2)], rows, {"s": Ragged2D(3 * B + 1, int(n.sum()) + 5)},
                slot, row)


def _max_len():
    lens = [3, 4, 5, 0, None, 5, 4] * 11
    cols = [("p", I1), ("a", I1), ("q", F1)]
    rows = [{"p": [[1, 2, 3] if k % 3 else [1] for k in range(len(lens))],
             "a": [None if n is None else list(range(n)) for n in lens],
             "q": [[7] * (1 + k % 4) for k in range(len(lens))]}]
    specs = {"p": Padded(2, truncate=True), "a": Ragged(max_len=4),
             "q": Padded(3, truncate=True)}
    return make(cols, rows, specs, np.zeros(len(lens)),
                np.arange(len(lens))[::-1])


def _int32(bad=None):
    """All int32 specs over the extremes; bad=(column, row, value) breaks one."""
    R = 70
    cols = [("x", I1), ("d", I1), ("y", I1), ("z", I2), ("w", I1)]
    rows = [{"x": [[LO, k] for k in range(R)],
             "d": [None if k % 3 else [HI] for k in range(R)],
             "y": [[HI, -k, LO][:k % 4] for k in range(R)],
             "z": [[[k, LO], [HI]][:k % 3] for k in range(R)],
             "w": [[LO, HI, k][:k % 4] for k in range(R)]}]
    for name, r, v in [bad] if bad else []:
        cell = rows[0][name][r]
        (cell[0] if name == "z" else cell)[0] = v
    specs = {"x": FixedLen(2, dtype="int32"),
             "d": FixedLen(default=LO, dtype="int32"),
             "y": Padded(3, pad=HI, dtype="int32"),
             "z": Padded2D(2, 2, pad=-1, dtype="int32"),
             "w": Ragged(capacity=3 * R + 1, dtype="int32")}
    return make(cols, rows, specs, np.zeros(R), (np.arange(R) * 3) % R)


EMPTY_RUNS = [1000] + [0] * 70 + [24] + [0] * 70 + [5] + [0] * 70 + \
    [2500, 3, 0, 7]
CASES = {f"scan-B{B}": functools.partial(_scan, B)
         for B in (1, 63, 64, 65, 255, 256, 257, 1025)}
CASES.update({
    "gather-long-row-and-empty-runs": lambda: _gather(EMPTY_RUNS),
    "gather-all-empty": lambda: _gather([0] * 5),
    "bytes-misalignment": _bytes,
    "capacity-exact": lambda: _scan(65, (0,) * 5),
    "max-len": _max_len,
    "int32": _int32,
})
for k, n in enumerate(("ragged", "bytes-items", "bytes-values", "list-items",
                       "list-values")):  # total == that capacity + 1
    CASES[f"capacity-{n}"] = functools.partial(
        _scan, 65, (3, 2, 5, 1, 3)[:k] + (-1,) + (3, 2, 5, 1, 3)[k + 1:])
for bad in (("x", 9, HI + 1), ("y", 11, LO - 1), ("z", 5, HI + 1),
            ("w", 7, LO - 1)):
    CASES[f"int32-range-{bad[0]}"] = functools.partial(_int32, bad)


case = functools.lru_cache(maxsize=None)(lambda name: CASES[name]())


@pytest.mark.parametrize("name", list(CASES))
def test_host_core_matches_reference(name):
    c, st0 = case(name), check(case(name), "cpu")
    cause = (RANGE if name.startswith("int32-range") else CAPACITY
             if name.startswith("capacity-") and "exact" not in name else 0)
    assert (0 if st0 == STATUS_CLEAN else st0 & 0xFF) == cause
    if cause:
        col = list(c["specs"])[(st0 >> 8) & 0xFF]
        with pytest.raises(ValueError,
                           match=f"'{col}'.*batch row {st0 >> 16} "):
            collate_batch(c["sources"], c["slot"], c["row"], c["specs"])


@pytest.mark.parametrize("name,spec", [
    ("a", FixedLen(default=HI + 1, dtype="int32")),
    ("a", Padded(2, pad=LO - 1, dtype="int32")),
    ("l", Padded2D(2, 2, pad=2**40, dtype="int32")),
    ("f", Ragged(capacity=8, dtype="int32")),
    ("s", Ragged2D(4, 8, dtype="int32")),
    ("a", Ragged(capacity=8, dtype="int16")),
    ("a", Ragged()),
    ("a", Ragged(capacity=0)),
    ("a", Ragged(max_len=2**31)),
    ("s", Ragged2D(2**31, 8)),
    ("l", Ragged2D(4, 2.5)),
    ("l", Ragged(capacity=8)),      # one-level spec on a FeatureList
    ("a", Ragged2D(4, 8)),          # two-level spec on a flat column
])
def test_bad_specs_are_rejected_on_the_host(name, spec):
    with pytest.raises(ValueError, match=f"'{name}'"):
        plan_columns(C.schema_of(COLS), {name: spec})
