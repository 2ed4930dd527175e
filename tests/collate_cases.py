"""Shared cases for the collation tests (no tests here).

A case holds a window of small RecordBatches (numpy wire form, built here
directly from Python lists), a selection of (slot, row) pairs, the specs, and
what the batch must be: the dense outputs, or the first bad cell. The
expectation comes from `reference` below, written from the words of the spec
in plain loops over Python lists; it shares nothing with csrc/collate_core.h.

Rows are Python values: None (absent), a list of numbers (one level), a list
of lists of numbers (FeatureList) or a list of bytes objects (bytes column).
Floats travel as their uint32 bit patterns, so NaN payloads and negative zero
are compared exactly.
"""

import functools
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

import spark_tfrecord_amd as stf
from spark_tfrecord_amd.collate import FixedLen, Padded, Padded2D
from spark_tfrecord_amd.columnar import RecordBatch, WireColumn
from spark_tfrecord_amd.schema import KIND_BYTES, KIND_FLOAT, KIND_INT64

MISSING, LENGTH = 1, 2  # cause codes of csrc/collate_core.h

# column shapes: (wire kind, levels)
I1, F1 = ("i", 1), ("f", 1)       # ArrayType(Long) / ArrayType(Float)
I0 = ("i", 0)                     # LongType scalar (one value per row)
I2, F2 = ("i", 2), ("f", 2)       # FeatureList of Int64List / FloatList
S2 = ("s", 2)                     # ArrayType(String): row -> strings -> bytes

_TYPES = {
    I0: lambda: stf.LongType(),
    I1: lambda: stf.ArrayType(stf.LongType()),
    F1: lambda: stf.ArrayType(stf.FloatType()),
    I2: lambda: stf.ArrayType(stf.ArrayType(stf.LongType())),
    F2: lambda: stf.ArrayType(stf.ArrayType(stf.FloatType())),
    S2: lambda: stf.ArrayType(stf.StringType()),
}
_KIND = {"i": KIND_INT64, "f": KIND_FLOAT, "s": KIND_BYTES}

FLOAT_ODDITIES = [0x7FC12345, 0x80000000, 0xFFC00001, 0x7F800000, 0x00000001]


def fbits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


# ---------------------------------------------------------------------------
# wire form from Python rows
# ---------------------------------------------------------------------------

def wire_column(shape, rows) -> WireColumn:
    kind, levels = shape
    R = len(rows)
    presence = np.array([0 if r is None else 1 for r in rows], np.uint8)
    row_off, list_off, sub_off, elem_off = [0], [0], [0], None
    flat = []
    if kind == "s":
        # one junk byte in front and odd lengths: strings start at odd offsets
        blob = bytearray(b"\xEE")
        elem_off = [1]
        for r in rows:
            for s in (r or []):
                blob += s
                elem_off.append(len(blob))
            row_off.append(len(elem_off) - 1)
        values = np.frombuffer(bytes(blob), np.uint8).copy()
        return WireColumn(KIND_BYTES, False, presence,
                          np.array(row_off, np.int64), values,
                          elem_off=np.array(elem_off, np.int64))
    for r in rows:
        if levels == 2:
            for sub in (r or []):
                flat.extend(sub)
                sub_off.append(len(flat))
            list_off.append(len(sub_off) - 1)
        elif r is not None:
            flat.extend(r if levels == 1 else [r[0]] if r else [])
        row_off.append(len(flat))
    if kind == "i":
        values = np.array(flat, np.int64).reshape(-1)
    else:
        values = np.array(flat, np.uint32).reshape(-1).view(np.float32)
    if levels == 2:
        return WireColumn(_KIND[kind], True, presence,
                          np.array(row_off, np.int64), values,
                          list_off=np.array(list_off, np.int64),
                          sub_off=np.array(sub_off, np.int64))
    return WireColumn(_KIND[kind], False, presence,
                      np.array(row_off, np.int64), values)


def schema_of(cols) -> "stf.StructType":
    return stf.StructType([stf.StructField(n, _TYPES[shape](), True)
                           for n, shape in cols])


# ---------------------------------------------------------------------------
# the reference: the spec's words over Python lists
# ---------------------------------------------------------------------------

def _pad_value(shape, v):
    return fbits(float(v)) if shape[0] == "f" else int(v)


def _padded(vals, L, pad, truncate):
    """-> (L values, len, truncated, error)"""
    n = len(vals)
    if n > L:
        if not truncate:
            return list(vals[:L]), L, False, LENGTH
        return list(vals[:L]), L, True, 0
    return list(vals) + [pad] * (L - n), n, False, 0


def reference_cell(shape, spec, row):
    """One (column, row) -> (dict of per-row outputs, truncated, cause)."""
    if isinstance(spec, FixedLen):
        K = 1 if spec.length is None else spec.length
        vals = [] if row is None else list(row)
        if len(vals) == 0:
            if spec.default is None:
                return {"": [0] * K}, False, MISSING
            return {"": [_pad_value(shape, spec.default)] * K}, False, 0
        if len(vals) != K:
            return {"": [0] * K}, False, LENGTH
        return {"": vals}, False, 0
    pad = _pad_value(shape, spec.pad)
    if isinstance(spec, Padded):
        vals = [] if row is None else list(row)
        out, n, tr, err = _padded(vals, spec.max_len, pad, spec.truncate)
        return {"": out, "_len": n}, tr, err
    T, L = spec.max_outer, spec.max_inner
    items = [] if row is None else [list(x) for x in row]
    trunc = False
    cause = 0
    if len(items) > T:
        if spec.truncate:
            trunc = True
        else:
            cause = LENGTH
        items = items[:T]
    grid, lens = [], []
    for t in range(T):
        if t < len(items):
            out, n, tr, err = _padded(items[t], L, pad, spec.truncate)
            trunc |= tr
            cause = cause or err
        else:
            out, n = [pad] * L, 0
        grid.append(out)
        lens.append(n)
    return {"": grid, "_outer": len(items), "_len": lens}, trunc, cause


_OUT_DTYPE = {"i": np.int64, "f": np.uint32, "s": np.uint8}


@dataclass
class Case:
    name: str
    cols: list                 # [(name, shape)]
    rows: list                 # rows[slot][column name] -> list of rows
    specs: Dict[str, object]   # ordered as given
    sel_slot: np.ndarray
    sel_row: np.ndarray
    sources: list = field(default=None)
    expect: Optional[dict] = None         # name -> array (None on an error)
    expect_error: Optional[tuple] = None  # (b, column index, cause)
    expect_truncated: int = 0

    def finish(self):
        schema = schema_of(self.cols)
        self.sources = [
            RecordBatch(schema,
                        [wire_column(shape, slot[n]) for n, shape in self.cols],
                        len(slot[self.cols[0][0]]))
            for slot in self.rows]
        shapes = dict(self.cols)
        acc = {}
        first_err = None
        trunc_rows = 0
        for b, (s, r) in enumerate(zip(self.sel_slot, self.sel_row)):
            row_tr = False
            for c, (name, spec) in enumerate(self.specs.items()):
                outs, tr, cause = reference_cell(
                    shapes[name], spec, self.rows[s][name][r])
                row_tr |= tr
                if cause and first_err is None:
                    first_err = (b, c, cause)
                for suffix, v in outs.items():
                    acc.setdefault(name + suffix, []).append(v)
            trunc_rows += row_tr
        if first_err is not None:
            self.expect_error = first_err
            return self
        self.expect_truncated = trunc_rows
        self.expect = {}
        for name, spec in self.specs.items():
            dt = _OUT_DTYPE[shapes[name][0]]
            v = np.array(acc[name], dt)
            if isinstance(spec, FixedLen) and spec.length is None:
                v = v.reshape(-1)
            if dt == np.uint32:
                v = v.view(np.float32)
            self.expect[name] = v
            for suffix in ("_len", "_outer"):
                if name + suffix in acc:
                    self.expect[name + suffix] = np.array(acc[name + suffix],
                                                          np.int32)
        return self


# ---------------------------------------------------------------------------
# row generators
# ---------------------------------------------------------------------------

def _num(rng, kind):
    if kind == "f":
        if rng.random() < 0.15:
            return FLOAT_ODDITIES[int(rng.integers(len(FLOAT_ODDITIES)))]
        return fbits(float(rng.standard_normal()))
    return int(rng.integers(-2**62, 2**62))


def _vals(rng, kind, n):
    if kind == "s":
        return bytes(rng.integers(1, 256, n, dtype=np.uint8).tolist())
    return [_num(rng, kind) for _ in range(n)]


def rows_1level(rng, shape, R, L, *, absent=True, empty=True, over=False,
                exact_only=False):
    """Counts cycle through: absent, 0 values, exactly L, L+1 (when `over`),
    and random counts in 0..L."""
    kind = shape[0]
    out = []
    for r in range(R):
        if exact_only:
            out.append(_vals(rng, kind, L))
            continue
        pick = (r + int(rng.integers(2))) % 6
        if pick == 0 and absent:
            out.append(None)
        elif pick == 1 and empty:
            out.append([])
        elif pick == 2 or not (absent or empty):
            out.append(_vals(rng, kind, L))
        elif pick == 3 and over:
            out.append(_vals(rng, kind, L + 1 + int(rng.integers(3))))
        else:
            n = int(rng.integers(0 if empty else 1, L + 1))
            out.append(_vals(rng, kind, n))
    return out


def rows_fixed_default(rng, shape, R, K):
    """Absent, empty or exactly K values."""
    out = []
    for r in range(R):
        pick = r % 3
        out.append(None if pick == 0 else [] if pick == 1
                   else _vals(rng, shape[0], K))
    return out


def rows_2level(rng, shape, R, T, L, *, over=False):
    """Outer counts: absent, 0, T, more than T (when `over`), random; inner
    lists: empty, exactly L, longer than L (when `over`), random."""
    kind = shape[0]

    def inner():
        pick = int(rng.integers(5))
        if pick == 0:
            n = 0
        elif pick == 1:
            n = L
        elif pick == 2 and over:
            n = L + 1 + int(rng.integers(4))
        else:
            n = int(rng.integers(0, L + 1))
        return _vals(rng, kind, n)

    out = []
    for r in range(R):
        pick = (r + int(rng.integers(2))) % 5
        if pick == 0:
            out.append(None)
            continue
        if pick == 1:
            oc = 0
        elif pick == 2:
            oc = T
        elif pick == 3 and over:
            oc = T + 1 + int(rng.integers(2))
        else:
            oc = int(rng.integers(0, T + 1))
        out.append([inner() for _ in range(oc)])
    return out


def _selection(rng, B, slot_rows):
    """Random (slot, row) pairs with repeats over the non-empty slots."""
    ok = [s for s, n in enumerate(slot_rows) if n]
    slot = rng.choice(ok, B).astype(np.int32)
    row = np.array([rng.integers(slot_rows[s]) for s in slot], np.int64)
    return slot, row


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

BS = [1, 63, 64, 65, 257]
LS = [1, 3, 8, 64, 65]
TS = [1, 2, 5]
BYTE_LS = [1, 7, 8, 12, 17]


def _case_1level(B, L, seed):
    rng = np.random.default_rng(seed)
    slot_rows = [max(3, B // 2), 7]
    cols = [("fix_i", I1), ("fix_f", F1), ("pad_i", I1), ("pad_f", F1)]
    rows = [{
        "fix_i": rows_1level(rng, I1, R, L, exact_only=True),
        "fix_f": rows_fixed_default(rng, F1, R, L),
        "pad_i": rows_1level(rng, I1, R, L),
        "pad_f": rows_1level(rng, F1, R, L, over=True),
    } for R in slot_rows]
    specs = {"fix_i": FixedLen(L), "fix_f": FixedLen(L, default=-1.5),
             "pad_i": Padded(L, pad=-7), "pad_f": Padded(L, pad=0.5,
                                                         truncate=True)}
    slot, row = _selection(rng, B, slot_rows)
    return Case(f"one-level-B{B}-L{L}", cols, rows, specs, slot, row).finish()


def _case_2level(B, T, L, seed, tag=""):
    rng = np.random.default_rng(seed)
    slot_rows = [max(4, B // 3), 9]
    cols = [("seq_i", I2), ("seq_f", F2)]
    rows = [{
        "seq_i": rows_2level(rng, I2, R, T, L),
        "seq_f": rows_2level(rng, F2, R, T, L, over=True),
    } for R in slot_rows]
    specs = {"seq_i": Padded2D(T, L, pad=-1),
             "seq_f": Padded2D(T, L, pad=0.25, truncate=True)}
    slot, row = _selection(rng, B, slot_rows)
    return Case(f"featurelist{tag}-B{B}-T{T}-L{L}", cols, rows, specs, slot,
                row).finish()


def _case_bytes(B, T, L, seed, tag=""):
    rng = np.random.default_rng(seed)
    slot_rows = [max(4, B // 3), 9]
    cols = [("str", S2), ("str_cut", S2)]
    rows = [{
        "str": rows_2level(rng, S2, R, T, L),
        "str_cut": rows_2level(rng, S2, R, T, L, over=True),
    } for R in slot_rows]
    specs = {"str": Padded2D(T, L, pad=0x20),
             "str_cut": Padded2D(T, L, pad=0, truncate=True)}
    slot, row = _selection(rng, B, slot_rows)
    return Case(f"bytes{tag}-B{B}-T{T}-L{L}", cols, rows, specs, slot,
                row).finish()


def _case_column_table():
    """Six columns of different modes and sizes in one call; rows interleave
    three slots of different row counts around an empty slot, with repeats.
    `id` is smaller than one block (65 units), `big` spans many (21125)."""
    rng = np.random.default_rng(77)
    B = 65
    slot_rows = [5, 0, 40, 17]
    cols = [("id", I0), ("ints", I1), ("floats", F1), ("big", F2),
            ("tokens", S2), ("steps", I2)]
    rows = [{
        "id": [[_num(rng, "i")] for _ in range(R)],
        "ints": rows_1level(rng, I1, R, 8, over=True),
        "floats": rows_1level(rng, F1, R, 16, exact_only=True),
        "big": rows_2level(rng, F2, R, 5, 65, over=True),
        "tokens": rows_2level(rng, S2, R, 2, 12, over=True),
        "steps": rows_2level(rng, I2, R, 3, 4),
    } for R in slot_rows]
    specs = {"id": FixedLen(), "ints": Padded(8, truncate=True),
             "floats": FixedLen(16), "big": Padded2D(5, 65, truncate=True),
             "tokens": Padded2D(2, 12, pad=0x2E, truncate=True),
             "steps": Padded2D(3, 4, pad=-9)}
    slot = np.array([(0, 2, 3)[b % 3] for b in range(B)], np.int32)
    row = np.array([(b * 7) % slot_rows[s] for b, s in enumerate(slot)],
                   np.int64)
    row[10] = row[13] = row[16]  # slot 2, same row three times
    return Case("column-table", cols, rows, specs, slot, row).finish()


def _error_case(name, cols, specs, good, bad_cells, B=70):
    """`good[name]` makes a valid row; `bad_cells` = {(b, name): row}. One
    slot, batch row b reads row b."""
    rows = [{n: [good[n]() for _ in range(B)] for n, _ in cols}]
    for (b, n), v in bad_cells.items():
        rows[0][n][b] = v
    return Case(name, cols, rows, specs, np.zeros(B, np.int32),
                np.arange(B, dtype=np.int64)).finish()


def _error_cases():
    cols = [("a", I1), ("b", F1), ("c", I2), ("d", S2)]
    specs = {"a": FixedLen(2), "b": Padded(3), "c": Padded2D(2, 2),
             "d": Padded2D(1, 4)}
    good = {"a": lambda: [1, 2], "b": lambda: [fbits(1.0)],
            "c": lambda: [[5], [6, 7]], "d": lambda: [b"abc"]}
    out = [
        # two bad cells: the first in (b, column) order wins, whichever
        # column or block sees it first
        _error_case("err-two-cells-b-order", cols, specs, good,
                    {(40, "a"): [1], (12, "d"): [b"toolong"]}),
        _error_case("err-two-cells-column-order", cols, specs, good,
                    {(12, "c"): [[1], [2], [3]], (12, "b"): [0, 0, 0, 0]}),
        _error_case("err-missing-absent", cols, specs, good,
                    {(69, "a"): None}),
        _error_case("err-missing-empty", cols, specs, good, {(0, "a"): []}),
        _error_case("err-fixed-length", cols, specs, good,
                    {(33, "a"): [1, 2, 3]}),
        _error_case("err-padded-length", cols, specs, good,
                    {(64, "b"): [fbits(2.0)] * 4}),
        _error_case("err-2d-outer-length", cols, specs, good,
                    {(5, "c"): [[1], [2], [3]]}),
        _error_case("err-2d-inner-length", cols, specs, good,
                    {(6, "c"): [[1], [2, 3, 4]]}),
        _error_case("err-bytes-inner-length", cols, specs, good,
                    {(7, "d"): [b"12345"]}),
    ]
    # the same absent / empty rows pass once the spec has a default
    specs_d = dict(specs, a=FixedLen(2, default=-3))
    out.append(_error_case("missing-with-default", cols, specs_d, good,
                           {(69, "a"): None, (0, "a"): []}))
    assert out[-1].expect_error is None
    assert out[0].expect_error == (12, 3, LENGTH)
    assert out[1].expect_error == (12, 1, LENGTH)
    assert out[2].expect_error == (69, 0, MISSING)
    return out


def _counter_case():
    """truncated_rows counts rows: row 3 is cut in two columns and in
    several cells of one, row 9 in one cell."""
    cols = [("p", I1), ("q", F2), ("s", S2)]
    specs = {"p": Padded(2, truncate=True), "q": Padded2D(2, 2, truncate=True),
             "s": Padded2D(1, 3, truncate=True)}
    good = {"p": lambda: [1], "q": lambda: [[fbits(1.0)]],
            "s": lambda: [b"ab"]}
    f = fbits(3.0)
    case = _error_case("counter-rows-not-cells", cols, specs, good, {
        (3, "p"): [1, 2, 3],
        (3, "q"): [[f, f, f], [f, f, f, f], [f]],
        (3, "s"): [b"abcdef", b"x"],
        (9, "q"): [[f], [f, f, f]],
    }, B=12)
    assert case.expect_truncated == 2
    return case


@functools.lru_cache(maxsize=None)
def all_cases() -> List[Case]:
    """Every case, built once per process."""
    cases = []
    seed = 1000
    for B in BS:
        for L in LS:
            seed += 1
            cases.append(_case_1level(B, L, seed))
    # every (T, L) pair with the Bs in rotation, then every B at one pair
    for i, (T, L) in enumerate((T, L) for T in TS for L in LS):
        seed += 1
        cases.append(_case_2level(BS[i % len(BS)], T, L, seed))
    for B in BS:
        seed += 1
        cases.append(_case_2level(B, 2, 3, seed, "-everyB"))
    for i, (T, L) in enumerate((T, L) for T in TS for L in BYTE_LS):
        seed += 1
        cases.append(_case_bytes(BS[(i + 2) % len(BS)], T, L, seed))
    for B in BS:
        seed += 1
        cases.append(_case_bytes(B, 2, 12, seed, "-everyB"))
    cases.append(_case_column_table())
    cases.extend(_error_cases())
    cases.append(_counter_case())
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


def case_names() -> List[str]:
    return [c.name for c in all_cases()]


def case(name: str) -> Case:
    return next(c for c in all_cases() if c.name == name)
