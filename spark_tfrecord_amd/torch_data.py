"""Training-pipeline integration: TFRecord shards as a torch IterableDataset.

The reference stops at Spark DataFrames; the MI355X-native equivalent of
"TFRecord -> accelerator" is streaming decoded shards straight into device
tensors (decode happens ON the training GPU — bytes cross PCIe once, columns
never touch host). Files are the sharding unit (matching the reference's
one-task-per-file model, DefaultSource.scala:26-29): they are split across
torch.distributed ranks and DataLoader workers round-robin.

    ds = TFRecordIterableDataset(path, batch_rows=8192)
    for batch in ds:           # dict: name -> values tensor,
        ...                    #       name+"_offsets" -> row offsets (ragged)

TFRecordBatchDataset goes the rest of the way: dense, shuffled batches of a
fixed size, collated on the device from a window of decoded shards
(collate.py; one kernel launch and one host wait per batch).

    ds = TFRecordBatchDataset(path, features={"id": FixedLen(),
                                              "ints": Padded(8)},
                              batch_size=8192, shuffle_window=4)
    for batch in ds:           # dict: name -> [B], [B, L] or [B, T, L]
        ...
"""

from __future__ import annotations

import os
from typing import Any, Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import engine as engine_mod
from .infer import byte_array_schema
from .io import paths as P
from .schema import KIND_BYTES, StructType
from .columnar import RecordBatch
from .collate import (STATUS_CLEAN, Collator, FixedLen, Padded, Padded2D,
                      plan_columns)

__all__ = ["TFRecordIterableDataset", "TFRecordBatchDataset", "FixedLen",
           "Padded", "Padded2D"]


def _as_torch(x, device):
    if isinstance(x, torch.Tensor):
        return x if device is None else x.to(device)
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t if device is None else t.to(device)


def _slice_col(col, lo: int, hi: int, device):
    """Row-range [lo, hi) of one wire column as torch tensors."""
    row_off = _as_torch(col.row_off, None)
    v0 = int(row_off[lo])
    v1 = int(row_off[hi])
    out = {
        "offsets": _as_torch(col.row_off, device)[lo:hi + 1] - v0,
        "presence": _as_torch(col.presence, device)[lo:hi],
    }
    values = _as_torch(col.values, device)
    if col.kind == KIND_BYTES:
        elem_off = _as_torch(col.elem_off, None)
        b0 = int(elem_off[v0])
        b1 = int(elem_off[v1])
        out["values"] = values[b0:b1]
        out["value_offsets"] = _as_torch(col.elem_off, device)[v0:v1 + 1] - b0
    else:
        out["values"] = values[v0:v1]
    if col.is_seq and col.list_off is not None:
        list_off = _as_torch(col.list_off, None)
        l0 = int(list_off[lo])
        l1 = int(list_off[hi])
        out["list_offsets"] = _as_torch(col.list_off, device)[lo:hi + 1] - l0
        sub = _as_torch(col.sub_off, device)[l0:l1 + 1]
        out["sub_offsets"] = sub - sub[0]
    return out


class _ShardSource(torch.utils.data.IterableDataset):
    """What both datasets share: the file list and schema, the assignment of
    shards to ranks and workers, the per-shard decode dispatch and the
    prefetch thread."""

    shuffle_files = False
    seed = 0

    def _init_source(self, path, schema, record_type, engine, verify_crc,
                     prefetch, foreign_gzip):
        self.path = path
        self.record_type = record_type
        self.engine = engine
        self.verify_crc = verify_crc
        self.prefetch = int(prefetch)  # shards decoded ahead (0 = sync)
        # "device": other writers' gzip shards inflate on the GPU too
        # (read_tfrecord's option of the same name); checked here, resolved
        # against the engine in __iter__
        if foreign_gzip is not None:
            from .io.reader import FOREIGN_GZIP_MODES
            if str(foreign_gzip).lower() not in FOREIGN_GZIP_MODES:
                raise ValueError(
                    f"Unsupported foreign gzip mode {foreign_gzip!r} "
                    f"(expected one of {FOREIGN_GZIP_MODES})")
        self.foreign_gzip = foreign_gzip
        files = P.list_data_files(path)
        if not files:
            raise FileNotFoundError(f"No TFRecord files found under {path}")
        self.files: List[str] = files
        if schema is None:
            if record_type == "ByteArray":
                schema = byte_array_schema()
            else:
                from .io.reader import infer_schema_of_paths
                schema = infer_schema_of_paths(
                    files, record_type,
                    engine_mod.resolve_engine(engine)
                    if engine != "auto" else "cpu")
        self.schema = schema

    # -- sharding ---------------------------------------------------------
    def _my_files(self) -> List[str]:
        files = list(self.files)
        if self.shuffle_files:
            rng = np.random.default_rng(self.seed)
            rng.shuffle(files)
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                files = files[dist.get_rank()::dist.get_world_size()]
        except Exception:
            pass
        info = torch.utils.data.get_worker_info()
        if info is not None:
            files = files[info.id::info.num_workers]
        return files

    _foreign_device = False

    def _decode_one(self, fpath: str, eng: str, sub_schema):
        if os.path.getsize(fpath) == 0:
            return None
        if eng == "gpu" and P.codec_from_path(fpath) is None:
            from .engine import gpu as gpu_engine
            batch = gpu_engine.read_file_to_batch(
                fpath, sub_schema, self.record_type, self.verify_crc)
            torch.cuda.current_stream().synchronize()  # hand off across threads
            return batch
        if eng == "gpu":
            # compressed shards the device takes (gpu.device_source) inflate
            # or decode ON the training GPU; None -> host codec below
            from .engine import gpu as gpu_engine
            dev = gpu_engine.read_file_image(fpath, self._foreign_device)
            if dev is not None:
                if dev.numel() == 0:
                    return None
                off, lens = gpu_engine.scan_frames_device(dev)
                batch = gpu_engine.decode_device(
                    dev, off, lens, sub_schema, self.record_type,
                    self.verify_crc)
                torch.cuda.current_stream().synchronize()
                return batch
        from .engine import cpu as cpu_engine
        data = np.frombuffer(P.decompress_file(fpath), np.uint8)
        if data.size == 0:
            return None
        return cpu_engine.decode_buffer(data, sub_schema, self.record_type,
                                        self.verify_crc)

    def _decoded_shards(self, eng: str, sub_schema):
        """Yields (path, RecordBatch) for this rank's and worker's non-empty
        shards, in order, decoded `prefetch` shards ahead."""
        from .io.reader import _resolve_foreign_gzip
        self._foreign_device = _resolve_foreign_gzip(self.foreign_gzip, eng)
        files = self._my_files()
        if self.prefetch <= 0:
            for fpath in files:
                batch = self._decode_one(fpath, eng, sub_schema)
                if batch is not None:
                    yield fpath, batch
            return
        # background prefetch: a worker thread decodes the next shard(s) on
        # its own CUDA stream while the consumer drains the current one
        import queue
        import threading

        q: "queue.Queue" = queue.Queue(maxsize=self.prefetch)
        SENTINEL = object()

        def worker():
            try:
                stream = (torch.cuda.Stream()
                          if eng == "gpu" and torch.cuda.is_available() else None)
                for fpath in files:
                    if stream is not None:
                        with torch.cuda.stream(stream):
                            b = self._decode_one(fpath, eng, sub_schema)
                    else:
                        b = self._decode_one(fpath, eng, sub_schema)
                    if b is not None:
                        q.put((fpath, b))
                q.put(SENTINEL)
            except BaseException as e:  # noqa: BLE001 — surface in consumer
                q.put(e)

        t = threading.Thread(target=worker, daemon=True)
        t.start()
        while True:
            item = q.get()
            if item is SENTINEL:
                break
            if isinstance(item, BaseException):
                raise item
            yield item


class TFRecordIterableDataset(_ShardSource):
    """Iterates dicts of tensors over a TFRecord dataset.

    Each yielded item covers up to `batch_rows` rows of one shard:
      {col: values, col+"_offsets": per-row value offsets,
       col+"_presence": u8 mask, and for string/seq columns also
       col+"_value_offsets" / col+"_list_offsets" / col+"_sub_offsets"}.

    `device` "cuda": files decode on the GPU and tensors stay device-resident.
    Files are sharded across dist ranks (rank r takes files r, r+W, ...)
    and then across DataLoader workers the same way.
    """

    def __init__(self, path: str, schema: Optional[StructType] = None,
                 record_type: str = "Example", batch_rows: int = 65536,
                 columns: Optional[Sequence[str]] = None,
                 engine: str = "auto", verify_crc: bool = True,
                 shuffle_files: bool = False, seed: int = 0,
                 prefetch: int = 1, foreign_gzip: Optional[str] = None):
        super().__init__()
        self.batch_rows = int(batch_rows)
        self.columns = list(columns) if columns else None
        self.shuffle_files = shuffle_files
        self.seed = seed
        self._init_source(path, schema, record_type, engine, verify_crc,
                          prefetch, foreign_gzip)

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        eng = engine_mod.resolve_engine(self.engine)
        fields = [f for f in self.schema.fields
                  if self.columns is None or f.name in self.columns]
        sub_schema = StructType(fields)
        for _, batch in self._decoded_shards(eng, sub_schema):
            yield from self._emit(batch, fields, None)

    def _emit(self, batch: RecordBatch, fields, device):
        R = batch.num_rows
        for lo in range(0, R, self.batch_rows):
            hi = min(R, lo + self.batch_rows)
            out: Dict[str, torch.Tensor] = {}
            for f, col in zip(fields, batch.columns):
                parts = _slice_col(col, lo, hi, device)
                out[f.name] = parts["values"]
                out[f.name + "_offsets"] = parts["offsets"]
                out[f.name + "_presence"] = parts["presence"]
                for k in ("value_offsets", "list_offsets", "sub_offsets"):
                    if k in parts:
                        out[f"{f.name}_{k}"] = parts[k]
            out["_num_rows"] = torch.tensor(hi - lo)
            yield out


class _Slot:
    """One decoded shard in the shuffle window."""

    __slots__ = ("path", "batch", "perm", "cursor", "retired")

    def __init__(self, path, batch, perm):
        self.path, self.batch, self.perm = path, batch, perm
        self.cursor = 0
        self.retired = False

    @property
    def left(self) -> int:
        return self.batch.num_rows - self.cursor


class TFRecordBatchDataset(_ShardSource):
    """Dense batches of exactly `batch_size` rows, shuffled through a window
    of decoded shards and collated per `features` (name -> FixedLen / Padded
    / Padded2D, see collate.py).

    The window holds up to `shuffle_window` decoded shards; each has a
    seeded permutation of its rows. A batch draws `batch_size` rows
    uniformly without replacement from all rows left in the window, and a
    drained shard is replaced by the next one before the next draw.
    `shuffle_window=0`: no shuffle, rows in file order, batches crossing
    shard boundaries. The sampler is host-side numpy seeded from (seed,
    epoch, rank, worker) and sees only the shards' row counts, so both
    engines yield the same batches in the same order. Shards are visited in
    listing order; only the spec'd columns are decoded.

    engine "gpu": shards decode on the device and stay there; per batch only
    the selection crosses the link, one kernel gathers every column, and the
    iterator waits once, on the status words. `truncated_rows` accumulates
    over an iteration; `last_stats` holds the last iteration's batches,
    kernel launches and host waits.
    """

    def __init__(self, path: str, features: Dict[str, Any],
                 batch_size: int = 8192, shuffle_window: int = 4,
                 seed: int = 0, drop_last: bool = False,
                 engine: str = "auto", schema: Optional[StructType] = None,
                 record_type: str = "Example", verify_crc: bool = True,
                 prefetch: int = 1, foreign_gzip: Optional[str] = None):
        super().__init__()
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if int(shuffle_window) < 0:
            raise ValueError(
                f"shuffle_window must be >= 0, got {shuffle_window}")
        self.batch_size = int(batch_size)
        self.shuffle_window = int(shuffle_window)
        self.seed = int(seed)
        self.drop_last = bool(drop_last)
        self.epoch = 0
        self.truncated_rows = 0
        self.last_stats = {"batches": 0, "launches": 0, "host_waits": 0}
        self._init_source(path, schema, record_type, engine, verify_crc,
                          prefetch, foreign_gzip)
        self.features = dict(features)
        plan_columns(self.schema, self.features)  # pairing errors, up front

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def _rng(self) -> np.random.Generator:
        rank = 0
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                rank = dist.get_rank()
        except Exception:
            pass
        info = torch.utils.data.get_worker_info()
        return np.random.default_rng(
            [self.seed, self.epoch, rank, info.id if info is not None else 0])

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        eng = engine_mod.resolve_engine(self.engine)
        sub_schema = StructType([f for f in self.schema.fields
                                 if f.name in self.features])
        co = Collator(sub_schema, self.features, eng)
        rng = self._rng()
        shuffle = self.shuffle_window > 0
        width = max(self.shuffle_window, 1)
        shards = self._decoded_shards(eng, sub_schema)
        live: List[_Slot] = []   # table order; retired slots stay to the
        dirty = True             # end of the batch that still reads them
        self.truncated_rows = 0
        stats = self.last_stats = {"batches": 0, "launches": 0,
                                   "host_waits": 0}

        def refill():
            nonlocal dirty
            while sum(not s.retired for s in live) < width:
                nxt = next(shards, None)
                if nxt is None:
                    return
                fpath, batch = nxt
                if eng == "gpu":
                    from .engine import gpu as gpu_engine
                    if not all(isinstance(c.presence, torch.Tensor)
                               and c.presence.is_cuda for c in batch.columns):
                        # a shard the host decoded (codec fallback)
                        batch = gpu_engine.batch_to_device(batch)
                perm = (rng.permutation(batch.num_rows) if shuffle
                        else np.arange(batch.num_rows, dtype=np.int64))
                live.append(_Slot(fpath, batch, perm.astype(np.int64)))
                dirty = True

        def finish(handle, slot, row, paths):
            outs, (st0, trunc) = co.finish(handle)
            if st0 != STATUS_CLEAN:
                b = st0 >> 16
                raise ValueError(
                    co.describe_error(st0, slot, row)
                    + f": shard {paths[int(slot[b])]}, row {int(row[b])}")
            self.truncated_rows += trunc
            stats["batches"] += 1
            stats["launches"] = co.launches
            stats["host_waits"] = co.host_waits
            return outs

        pending = None
        newest = None  # the last launch; the stream runs them in order
        try:
            refill()
            while True:
                sel_slot: List[np.ndarray] = []
                sel_row: List[np.ndarray] = []
                need = self.batch_size
                while need:
                    active = [i for i, s in enumerate(live) if not s.retired]
                    if not active:
                        break
                    left = np.array([live[i].left for i in active], np.int64)
                    k = min(need, int(left.sum()))
                    counts = (rng.multivariate_hypergeometric(left, k)
                              if len(active) > 1 else np.array([k]))
                    for i, n in zip(active, counts):
                        s = live[i]
                        n = int(n)
                        if n:
                            sel_slot.append(np.full(n, i, np.int32))
                            sel_row.append(s.perm[s.cursor:s.cursor + n])
                            s.cursor += n
                        if s.left == 0:
                            s.retired = True
                    need -= k
                    refill()
                if not sel_slot:
                    break
                slot = np.concatenate(sel_slot)
                row = np.concatenate(sel_row)
                if need and self.drop_last:
                    break
                if shuffle:
                    order = rng.permutation(slot.size)
                    slot, row = slot[order], row[order]
                if dirty:
                    co.set_window([s.batch for s in live])
                    dirty = False
                handle = newest = co.launch(slot, row)
                paths = [s.path for s in live]
                # a launched batch keeps its window alive, so the retired slots
                # can leave the table now; they are freed after its wait
                if any(s.retired for s in live):
                    live[:] = [s for s in live if not s.retired]
                    dirty = True
                # one batch ahead: this batch was drawn and launched while the
                # previous one ran; now wait for that one and hand it out
                if pending is not None:
                    yield finish(*pending)
                pending = (handle, slot, row, paths)
            if pending is not None:
                yield finish(*pending)
        finally:
            # leaving early (an error, or the consumer stopped): nothing may
            # be freed under a kernel that still reads it
            if newest is not None:
                co.abandon(newest)
