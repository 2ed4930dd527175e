"""Dense batches from ragged decoded shards: feature specs and the collator.

The decoder's wire form (columnar.py) is ragged: flat values plus offsets.
A model takes `[B]`, `[B, L]` or `[B, T, L]`. The specs below say, per column,
which dense shape a batch gets (modelled on tf.io.parse_example's
FixedLenFeature / VarLenFeature), and `collate_batch` gathers B rows, each a
(slot, row) pair into a window of decoded shards, into those tensors:

    FixedLen(length=None, default=None)   name: [B] or [B, K]
    Padded(max_len, pad=0, truncate=False)
                                          name: [B, L], name_len: int32 [B]
    Padded2D(max_outer, max_inner, pad=0, truncate=False)
                                          name: [B, T, L], name_outer: int32
                                          [B], name_len: int32 [B, T]

The semantics are csrc/collate_core.h's, run by the gfx950 kernel
(csrc/hip/collate.hip, one launch and one host wait per batch) or by the
same core in host loops (`_native.host_collate`).
"""

from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _native
from .columnar import RecordBatch, wire_fields
from .schema import (KIND_BYTES, KIND_FLOAT, KIND_INT64, NullType, StructType,
                     is_sequence_field, wire_kind_of)

__all__ = ["FixedLen", "Padded", "Padded2D", "Collator", "collate_batch",
           "plan_columns", "CAUSES"]

CM_FIXED, CM_PADDED, CM_PADDED2D = 0, 1, 2
CC_MISSING, CC_LENGTH = 1, 2
CAUSES = {CC_MISSING: "MISSING (row absent or empty and the spec has no "
                      "default)",
          CC_LENGTH: "LENGTH (row's value count does not fit the spec)"}
CF_DEFAULT, CF_TRUNCATE, CF_BYTES = 1, 2, 4
STATUS_CLEAN = (1 << 64) - 1

_SRC_WORDS = _native.COLLATE_SRC_WORDS
_COL_WORDS = _native.COLLATE_COL_WORDS
_TILE_UNITS = _native.COLLATE_TILE_UNITS
_MAX_COLS = _native.COLLATE_MAX_COLS


@dataclass(frozen=True)
class FixedLen:
    """Exactly `length` values per row (`None`: one value, output `[B]`).
    An absent or empty row takes `default` when one is given."""
    length: Optional[int] = None
    default: Optional[Union[int, float]] = None


@dataclass(frozen=True)
class Padded:
    """Up to `max_len` values per row, padded with `pad`; longer rows are cut
    when `truncate` is set and an error otherwise."""
    max_len: int
    pad: Union[int, float] = 0
    truncate: bool = False


@dataclass(frozen=True)
class Padded2D:
    """Up to `max_outer` items (lists of a FeatureList, or strings of a bytes
    column) of up to `max_inner` elements each."""
    max_outer: int
    max_inner: int
    pad: Union[int, float] = 0
    truncate: bool = False


_NP_DTYPE = {KIND_INT64: np.int64, KIND_FLOAT: np.float32, KIND_BYTES: np.uint8}
_TORCH_DTYPE = {KIND_INT64: torch.int64, KIND_FLOAT: torch.float32,
                KIND_BYTES: torch.uint8}
_ESIZE = {KIND_INT64: 8, KIND_FLOAT: 4, KIND_BYTES: 1}


def _fill_bits(kind: int, value, name: str) -> int:
    """`value` in the column's number format, as the low bytes of a word."""
    try:
        if kind == KIND_INT64:
            return struct.unpack("<Q", struct.pack("<q", int(value)))[0]
        if kind == KIND_FLOAT:
            return struct.unpack("<I", struct.pack("<f", float(value)))[0]
        return struct.unpack("<B", struct.pack("<B", int(value)))[0]
    except (struct.error, TypeError, ValueError) as e:
        raise ValueError(f"column '{name}': fill value {value!r} does not fit "
                         f"the column's type") from e


@dataclass(frozen=True)
class _Plan:
    """One spec checked against its schema field."""
    name: str
    index: int      # column position in the source batches
    kind: int
    mode: int
    T: int
    L: int
    fill: int
    flags: int
    squeeze: bool   # FixedLen(length=None): output [B], not [B, 1]

    def shapes(self, B: int) -> Dict[str, tuple]:
        """Output name -> (shape, numpy dtype) for a batch of B rows."""
        dt = _NP_DTYPE[self.kind]
        if self.mode == CM_FIXED:
            return {self.name: ((B,) if self.squeeze else (B, self.L), dt)}
        if self.mode == CM_PADDED:
            return {self.name: ((B, self.L), dt),
                    self.name + "_len": ((B,), np.int32)}
        return {self.name: ((B, self.T, self.L), dt),
                self.name + "_outer": ((B,), np.int32),
                self.name + "_len": ((B, self.T), np.int32)}


def _positive(v, what: str, name: str) -> int:
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 1:
        raise ValueError(f"column '{name}': {what} must be a positive integer, "
                         f"got {v!r}")
    return int(v)


def plan_columns(schema: StructType, features: Dict[str, Any]) -> List[_Plan]:
    """Check every spec against the schema; ValueError names the column."""
    if not features:
        raise ValueError("features: at least one column spec is needed")
    if len(features) > _MAX_COLS:
        raise ValueError(f"features: {len(features)} columns, the collator "
                         f"takes at most {_MAX_COLS}")
    wf = wire_fields(schema)
    by_name = {f.name: i for i, f in enumerate(wf)}
    plans = []
    for name, spec in features.items():
        if name not in by_name:
            null = any(f.name == name and isinstance(f.dataType, NullType)
                       for f in schema.fields)
            raise ValueError(
                f"column '{name}': " + ("a NullType column has no values to "
                                        "collate" if null
                                        else "not in the schema"))
        f = wf[by_name[name]]
        kind = wire_kind_of(f.dataType)
        seq = is_sequence_field(f.dataType)
        if isinstance(spec, (FixedLen, Padded)):
            if seq or kind == KIND_BYTES:
                raise ValueError(
                    f"column '{name}': {type(spec).__name__} takes an int64 "
                    f"or float column that is not a FeatureList, not "
                    f"{f.dataType.simple_string()}")
            if isinstance(spec, FixedLen):
                L = 1 if spec.length is None else _positive(
                    spec.length, "length", name)
                has = spec.default is not None
                plans.append(_Plan(
                    name, by_name[name], kind, CM_FIXED, 1, L,
                    _fill_bits(kind, spec.default if has else 0, name),
                    CF_DEFAULT if has else 0, spec.length is None))
            else:
                plans.append(_Plan(
                    name, by_name[name], kind, CM_PADDED, 1,
                    _positive(spec.max_len, "max_len", name),
                    _fill_bits(kind, spec.pad, name),
                    CF_TRUNCATE if spec.truncate else 0, False))
        elif isinstance(spec, Padded2D):
            if seq == (kind == KIND_BYTES):
                raise ValueError(
                    f"column '{name}': Padded2D takes a numeric FeatureList "
                    f"or a bytes column that is not a FeatureList, not "
                    f"{f.dataType.simple_string()}")
            plans.append(_Plan(
                name, by_name[name], kind, CM_PADDED2D,
                _positive(spec.max_outer, "max_outer", name),
                _positive(spec.max_inner, "max_inner", name),
                _fill_bits(kind, spec.pad, name),
                (CF_TRUNCATE if spec.truncate else 0)
                | (CF_BYTES if kind == KIND_BYTES else 0), False))
        else:
            raise ValueError(f"column '{name}': {spec!r} is not a FixedLen, "
                             f"Padded or Padded2D spec")
    return plans


def _ptr(x, np_dtype) -> int:
    if x is None:
        return 0
    if isinstance(x, torch.Tensor):
        return x.data_ptr() if x.numel() else 0
    return x.ctypes.data if x.size else 0


class Collator:
    """Collates batches out of a window of decoded shards.

    `set_window(sources)` takes the RecordBatches (device-resident for the
    GPU engine) and builds the descriptor table, uploading it for the GPU;
    `run(sel_slot, sel_row)` then makes one batch (`launch` + `finish`, which
    a caller may split to prepare the next batch under this one). The window
    is kept until the next `set_window`, and nothing in it is copied or
    concatenated.
    """

    def __init__(self, schema: StructType, features: Dict[str, Any],
                 engine: str = "cpu"):
        if engine not in ("cpu", "gpu"):
            raise ValueError(f"unknown engine {engine!r}")
        self.engine = engine
        self.plans = plan_columns(schema, features)
        self.launches = 0
        self.host_waits = 0
        self._sources: List[RecordBatch] = []
        self._keep: list = []
        self._rows = np.zeros(0, np.int64)
        self._src_table = None

    # -- window -----------------------------------------------------------
    def set_window(self, sources: Sequence[Optional[RecordBatch]]):
        gpu = self.engine == "gpu"
        keep = []
        table = np.zeros((len(sources), len(self.plans), _SRC_WORDS), np.int64)
        rows = np.zeros(len(sources), np.int64)
        for s, batch in enumerate(sources):
            if batch is None or batch.num_rows == 0:
                continue
            rows[s] = batch.num_rows
            for c, p in enumerate(self.plans):
                col = batch.columns[p.index]
                if col.kind != p.kind:
                    raise ValueError(
                        f"column '{p.name}': slot {s} holds wire kind "
                        f"{col.kind}, the schema says {p.kind}")
                parts = []
                for x, dt in ((col.presence, np.uint8),
                              (col.row_off, np.int64),
                              (col.values, _NP_DTYPE[p.kind]),
                              (col.elem_off, np.int64),
                              (col.list_off, np.int64),
                              (col.sub_off, np.int64)):
                    if x is not None:
                        if gpu:
                            if not (isinstance(x, torch.Tensor) and x.is_cuda):
                                raise ValueError(
                                    f"column '{p.name}': slot {s} is not "
                                    f"device-resident (engine='gpu')")
                            x = x.contiguous()
                            if x.dtype != getattr(torch, np.dtype(dt).name):
                                raise ValueError(
                                    f"column '{p.name}': slot {s} has a "
                                    f"buffer of dtype {x.dtype}")
                        else:
                            if isinstance(x, torch.Tensor):
                                x = x.cpu().numpy()
                            x = np.ascontiguousarray(x, dtype=dt)
                        keep.append(x)
                    parts.append(_ptr(x, dt))
                table[s, c] = parts
        self._sources = list(sources)
        self._keep = keep
        self._rows = rows
        if gpu:
            host = torch.from_numpy(table.reshape(-1)).pin_memory()
            self._src_table = host.to("cuda", non_blocking=True)
            self._keep.append(host)
        else:
            self._src_table = table.reshape(-1)

    # -- checks the launcher relies on --------------------------------------
    def _check_selection(self, sel_slot, sel_row):
        sel_slot = np.ascontiguousarray(sel_slot)
        sel_row = np.ascontiguousarray(sel_row)
        if sel_slot.ndim != 1 or sel_slot.shape != sel_row.shape:
            raise ValueError("sel_slot and sel_row must be 1-D and equally "
                             "long")
        if (sel_slot.dtype.kind not in "iu" or sel_row.dtype.kind not in "iu"):
            raise ValueError("sel_slot and sel_row must be integer arrays")
        B = sel_slot.shape[0]
        if B < 1:
            raise ValueError("a batch needs at least one row")
        bad = (sel_slot < 0) | (sel_slot >= len(self._rows))
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError(f"batch row {b}: slot {int(sel_slot[b])} out of "
                             f"range (window of {len(self._rows)})")
        bad = (sel_row < 0) | (sel_row >= self._rows[sel_slot])
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError(
                f"batch row {b}: row {int(sel_row[b])} out of range for slot "
                f"{int(sel_slot[b])} ({int(self._rows[sel_slot[b]])} rows)")
        for p in self.plans:
            if B * p.T * p.L >= 1 << 31:
                raise ValueError(f"column '{p.name}': {B}x{p.T}x{p.L} "
                                 f"elements do not fit one batch (2^31)")
        return sel_slot.astype(np.int32), sel_row.astype(np.int64), B

    def _outputs(self, B: int, out: Optional[dict]):
        gpu = self.engine == "gpu"
        want = {}
        for p in self.plans:
            want.update(p.shapes(B))
        if out is None:
            if gpu:
                return {k: torch.empty(shape, device="cuda",
                                       dtype=getattr(torch, np.dtype(dt).name))
                        for k, (shape, dt) in want.items()}
            return {k: torch.from_numpy(np.empty(shape, dt))
                    for k, (shape, dt) in want.items()}
        if set(out) != set(want):
            raise ValueError(f"out: expected tensors {sorted(want)}, got "
                             f"{sorted(out)}")
        for k, (shape, dt) in want.items():
            t = out[k]
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape
                    or t.dtype != getattr(torch, np.dtype(dt).name)
                    or not t.is_contiguous() or t.is_cuda != gpu):
                raise ValueError(
                    f"out['{k}']: expected a contiguous "
                    f"{'device' if gpu else 'host'} tensor of shape {shape} "
                    f"and dtype {np.dtype(dt).name}")
        return dict(out)

    def _col_table(self, B: int, outs: dict) -> (np.ndarray, int):
        table = np.zeros((len(self.plans), _COL_WORDS), np.uint64)
        tile0 = 0
        for c, p in enumerate(self.plans):
            esize = _ESIZE[p.kind]
            elems = B * p.T * p.L
            units = (elems + 7) // 8 if esize == 1 else elems
            ln = outs.get(p.name + "_len")
            outer = outs.get(p.name + "_outer")
            table[c] = [p.mode, esize, p.T, p.L, p.fill, p.flags,
                        outs[p.name].data_ptr(),
                        ln.data_ptr() if ln is not None else 0,
                        outer.data_ptr() if outer is not None else 0,
                        tile0, units, 0]
            tile0 += (units + _TILE_UNITS - 1) // _TILE_UNITS
        return table.view(np.int64).reshape(-1), tile0

    # -- one batch ----------------------------------------------------------
    def launch(self, sel_slot, sel_row, out: Optional[dict] = None):
        """Start one batch and return a handle for `finish`. Every check
        happens before the native call. The handle keeps the window it reads
        alive, so `set_window` may be called for the next batch before this
        one is finished. Engine "cpu" does the work here."""
        if self._src_table is None:
            raise ValueError("set_window() first")
        sel_slot, sel_row, B = self._check_selection(sel_slot, sel_row)
        outs = self._outputs(B, out)
        cols, ntiles = self._col_table(B, outs)
        if self.engine == "cpu":
            status = np.array([STATUS_CLEAN, 0], np.uint64)
            _native.host_collate(self._src_table, cols, sel_slot, sel_row,
                                 status)
            return (outs, status, None, None)
        # one upload: status init | sel_row | column table | sel_slot
        nc = cols.size
        words = 2 + B + nc + (B + 1) // 2
        host = torch.empty(words, dtype=torch.int64, pin_memory=True)
        h = host.numpy()
        h[0], h[1] = -1, 0
        h[2:2 + B] = sel_row
        h[2 + B:2 + B + nc] = cols
        h[2 + B + nc:].view(np.int32)[:B] = sel_slot
        dev = host.to("cuda", non_blocking=True)
        base = dev.data_ptr()
        stream = torch.cuda.current_stream()
        _native.gpu_collate_rows(
            self._src_table.data_ptr(), base + 8 * (2 + B),
            base + 8 * (2 + B + nc), base + 16, len(self.plans), B, ntiles,
            base, stream.cuda_stream)
        self.launches += 1
        back = torch.empty(2, dtype=torch.int64, pin_memory=True)
        back.copy_(dev[:2], non_blocking=True)
        done = torch.cuda.Event()
        done.record(stream)
        return (outs, back, done, (self._keep, self._src_table, dev))

    def finish(self, handle):
        """Wait for a launched batch -> (outputs, status): status[0] is
        STATUS_CLEAN or the first bad cell as (b << 16) | (column << 8) |
        cause, status[1] the truncated rows."""
        outs, status, done, _alive = handle
        if done is None:
            return outs, (int(status[0]), int(status[1]))
        done.synchronize()  # the batch's one host wait
        self.host_waits += 1
        st = status.numpy().view(np.uint64)
        return outs, (int(st[0]), int(st[1]))

    def abandon(self, handle):
        """Wait out a launched batch whose result is not wanted, so that what
        it reads and writes can be freed."""
        if handle[2] is not None:
            handle[2].synchronize()

    def run(self, sel_slot, sel_row, out: Optional[dict] = None):
        """launch + finish."""
        return self.finish(self.launch(sel_slot, sel_row, out))

    def describe_error(self, status0: int, sel_slot, sel_row) -> str:
        """Column, cause and (slot, row) of an error status word."""
        b, c, cause = status0 >> 16, (status0 >> 8) & 0xFF, status0 & 0xFF
        return (f"column '{self.plans[c].name}': "
                f"{CAUSES.get(cause, f'cause {cause}')} at batch row {b} "
                f"(slot {int(sel_slot[b])}, row {int(sel_row[b])})")


def collate_batch(sources: Sequence[Optional[RecordBatch]], sel_slot, sel_row,
                  specs: Dict[str, Any], engine: str = "cpu",
                  out: Optional[dict] = None, return_status: bool = False):
    """Collate the rows `(sel_slot[b], sel_row[b])` of `sources` into dense
    tensors per `specs` (host tensors for engine "cpu", device tensors for
    "gpu", whose sources must be device-resident).

    Raises ValueError for a bad selection or output before anything runs, and
    for a row that violates its spec; `return_status=True` returns
    `(outputs, (status0, truncated_rows))` without raising on the latter.
    """
    schema = next((s.schema for s in sources if s is not None), None)
    if schema is None:
        raise ValueError("sources: no decoded shard in the window")
    co = Collator(schema, specs, engine)
    co.set_window(sources)
    outs, status = co.run(sel_slot, sel_row, out)
    if return_status:
        return outs, status
    if status[0] != STATUS_CLEAN:
        raise ValueError(co.describe_error(status[0], sel_slot, sel_row))
    return outs
