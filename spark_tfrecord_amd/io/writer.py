"""Write path: DataFrame-shaped data -> TFRecord files on disk.

Mirrors the reference's write pipeline: save-mode handling,
optional partitionBy (dynamic `col=value/` directories, partition columns
stripped from the payload), per-shard part files, codec compression, and a
`_SUCCESS` marker — with the row->proto serde and framing done by the native
engine (CPU host codec or gfx950 kernels) instead of Catalyst + JVM classes.
"""

from __future__ import annotations

import logging
import os
import uuid
from typing import Dict, List, Optional, Sequence

import numpy as np
import pyarrow as pa

from .. import engine as engine_mod
from ..arrow_interop import schema_from_arrow, schema_to_arrow, table_to_batch
from ..columnar import RecordBatch
from ..engine import cpu as cpu_engine
from ..schema import BinaryType, StructType, validate_schema_for_record_type
from ..utils import IOMetrics, StageTimer
from . import paths as P

__all__ = ["write_tfrecord", "normalize_input"]

RECORD_TYPES = ("Example", "SequenceExample", "ByteArray")

_log = logging.getLogger(__name__)


def normalize_input(data, schema: Optional[StructType]) -> pa.Table:
    """Accept pyarrow Table/RecordBatch, pandas DataFrame, dict of columns,
    or list of row-dicts; return a pyarrow Table."""
    if isinstance(data, dict) and schema is not None:
        # build at the target types directly: inferring first and casting
        # after costs ~4.7x on nested python-list columns (ragged 2-D input)
        target = schema_to_arrow(schema)
        for f in target:
            if f.name not in data:
                raise KeyError(f"column '{f.name}' not found in input data")
        try:
            return pa.table({f.name: data[f.name] for f in target},
                            schema=target)
        except (pa.ArrowInvalid, pa.ArrowTypeError, pa.ArrowNotImplementedError):
            pass  # fall through to infer + cast
    if hasattr(data, "to_arrow_table"):  # our DataFrame wrapper
        table = data.to_arrow_table()
    elif isinstance(data, pa.Table):
        table = data
    elif isinstance(data, pa.RecordBatch):
        table = pa.Table.from_batches([data])
    elif hasattr(data, "__dataframe__") or str(type(data).__module__).startswith("pandas"):
        table = pa.Table.from_pandas(data, preserve_index=False)
    elif isinstance(data, dict):
        table = pa.table(data)
    elif isinstance(data, list):
        table = pa.Table.from_pylist(data)
    else:
        raise TypeError(f"Cannot write object of type {type(data).__name__}")
    if schema is not None:
        # cast columns to the requested logical types
        target = schema_to_arrow(schema)
        cols = []
        for f in target:
            if f.name not in table.column_names:
                raise KeyError(f"column '{f.name}' not found in input data")
            cols.append(table.column(f.name).cast(f.type))
        table = pa.table(cols, schema=target)
    return table


def _partition_dir_value(v) -> str:
    """Directory-safe `value` for a `col=value/` component: Hive default
    partition for nulls, Hive/Spark %XX escaping for special characters
    (a value containing '/', '=' or '%' must not alter the layout)."""
    if v is None:
        return "__HIVE_DEFAULT_PARTITION__"
    if isinstance(v, float) and v == int(v):
        return str(int(v))
    s = str(v)
    return P.escape_path_name(s) if s else "__HIVE_DEFAULT_PARTITION__"


def _factorize_partitions(table: pa.Table, partition_by: Sequence[str]):
    """Vectorized grouping: per-row partition code (np.int64) + the list of
    value tuples, combos[code] = (v1, v2, ...). Nulls map to the Hive
    default-partition value like Spark's dynamic partition insert."""
    import pyarrow.compute as pc

    idx_cols = []
    val_lists = []
    for c in partition_by:
        arr = table.column(c)
        if isinstance(arr, pa.ChunkedArray):
            # chunk(0) is zero-copy; combine_chunks deep-copies even for one
            arr = (arr.chunk(0) if arr.num_chunks == 1
                   else arr.combine_chunks() if arr.num_chunks
                   else pa.array([], arr.type))
        if isinstance(arr, pa.ChunkedArray):
            arr = arr.chunk(0) if arr.num_chunks else pa.array([], arr.type)
        de = arr.dictionary_encode()
        vals = de.dictionary.to_pylist()
        idx = pc.fill_null(de.indices, len(vals)).to_numpy(zero_copy_only=False)
        idx_cols.append(idx.astype(np.int64))
        val_lists.append(vals + [None])
    if len(idx_cols) == 1:
        # dictionary codes are already dense [0, n_values): no unique() pass
        return idx_cols[0], [(v,) for v in val_lists[0]]
    code = idx_cols[0].copy()
    for i in range(1, len(idx_cols)):
        code = code * len(val_lists[i]) + idx_cols[i]
    uniq, inv = np.unique(code, return_inverse=True)
    combos = []
    for u in uniq:
        rem = int(u)
        rev = []
        for vals in reversed(val_lists[1:]):
            rem, k = divmod(rem, len(vals))
            rev.append(vals[k])
        rev.append(val_lists[0][rem])
        combos.append(tuple(reversed(rev)))
    return inv.astype(np.int64), combos


# Rows per chunk of the pipelined single-shard write. Large enough that
# per-chunk encode launches amortize, small enough that the conversion /
# encode / file-append stages of consecutive chunks actually overlap.
_PIPE_CHUNK_ROWS = int(os.environ.get("TFREC_WRITE_CHUNK_ROWS", "131072"))


def _single_shard_pipelined(table: pa.Table, schema: StructType,
                            record_type: str, fpath: str, eng: str,
                            metrics: Optional[IOMetrics]):
    """Single part file, built in row chunks: while chunk k's bytes land in
    the temp file on IO worker threads, chunk k+1 converts (host) and
    encodes (GPU). TFRecord frames are freely concatenable, so chunked
    encodes produce the identical file.

    Appends are plain write() calls chained in submission order on the IO
    pool — on the GPU box a single-file write() streams at ~4.8 GB/s, and
    neither threaded same-file pwrite (inode-lock serialized) nor mmap
    stores (per-page fault cost, ~2.9 GB/s, no thread scaling) beat it
    (measured, exp/exp_pipewrite.py). The win here is the overlap: convert
    and encode of chunk k+1 run while chunk k's bytes stream out. Temp +
    atomic rename keeps write_file_atomic's torn-write guarantee (the
    reference inherits the same guarantee from Spark's task-commit
    protocol)."""
    R = table.num_rows
    pool = P.shared_pool()
    os.makedirs(os.path.dirname(fpath), exist_ok=True)
    tmp = P.hidden_tmp_path(fpath, f"tmp.{uuid.uuid4().hex[:8]}")
    fd = os.open(tmp, os.O_CREAT | os.O_WRONLY | os.O_TRUNC, 0o644)
    nbytes = 0
    prev_write = None
    tag_futs: Dict[str, object] = {}

    def _append(view, after):
        if after is not None:
            after.result()
        mv = view if isinstance(view, bytes) else memoryview(view).cast("B")
        n = 0
        while n < len(mv):
            n += os.write(fd, mv[n:])
        return n

    try:
        for ci, lo in enumerate(range(0, R, _PIPE_CHUNK_ROWS)):
            chunk = table.slice(lo, min(_PIPE_CHUNK_ROWS, R - lo))
            batch = table_to_batch(chunk, schema)
            if eng == "gpu":
                from ..engine import gpu as gpu_engine

                img = gpu_engine.encode_device(
                    gpu_engine.batch_to_device(batch), record_type)
                tag = f"encw{ci % 2}"
                prev = tag_futs.get(tag)
                if prev is not None:
                    prev.result()  # the tag's pinned buffer is being reused
                raw = gpu_engine.device_to_pinned_view(img, tag=tag)
            else:
                tag = None
                raw = cpu_engine.encode_batch(batch, record_type)
            nbytes += len(raw) if isinstance(raw, bytes) else raw.nbytes
            if tag is None and prev_write is not None and ci % 4 == 0:
                prev_write.result()  # bound in-flight encoded chunk buffers
            prev_write = pool.submit(_append, raw, prev_write)
            if tag is not None:
                tag_futs[tag] = prev_write
        if prev_write is not None:
            prev_write.result()
        os.fsync(fd)
    except BaseException:
        if prev_write is not None:
            try:
                prev_write.result()
            except BaseException:
                pass
        os.close(fd)
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    os.close(fd)
    os.replace(tmp, fpath)
    if metrics is not None:
        metrics.add(rows=R, nbytes=nbytes, files=1)


GZIP_ENGINES = ("host", "device")


def _resolve_gzip_engine(gzip_engine: Optional[str], eng: str,
                         codec: Optional[str]) -> bool:
    """True when gzip output is compressed in HBM (csrc/hip/deflate.hip)
    instead of by host zlib. None = the default: "host", or what
    TFREC_GZ_ENGINE says for GPU-engine writes. Only the gzip codec has a
    device compressor; for any other codec the choice is ignored."""
    explicit = gzip_engine is not None
    if not explicit:
        gzip_engine = (os.environ.get("TFREC_GZ_ENGINE", "host")
                       if eng == "gpu" else "host")
    val = str(gzip_engine).lower()
    if val not in GZIP_ENGINES:
        raise ValueError(
            f"Unsupported gzip engine {gzip_engine!r} (expected one of "
            f"{GZIP_ENGINES})")
    if val == "device" and eng != "gpu":
        raise ValueError(
            'gzip_engine="device" needs the GPU engine; this write resolved '
            f"to engine={eng!r}")
    return val == "device" and codec == "gzip"


SNAPPY_ENGINES = ("host", "device")


def _resolve_snappy_engine(snappy_engine: Optional[str], eng: str,
                           codec: Optional[str]) -> bool:
    """True when snappy output is compressed in HBM (csrc/hip/snappy_enc.hip)
    instead of by the library on the host. None = the default: "host", or
    what TFREC_SNAPPY_ENGINE says for GPU-engine writes. For any codec but
    snappy the choice is ignored. The device takes blocks of up to 1 MiB: a
    larger TFREC_SNAPPY_BLOCK is compressed on the host, with a log line."""
    explicit = snappy_engine is not None
    if not explicit:
        snappy_engine = (os.environ.get("TFREC_SNAPPY_ENGINE", "host")
                         if eng == "gpu" else "host")
    val = str(snappy_engine).lower()
    if val not in SNAPPY_ENGINES:
        raise ValueError(
            f"Unsupported snappy engine {snappy_engine!r} (expected one of "
            f"{SNAPPY_ENGINES})")
    if val == "device" and eng != "gpu":
        raise ValueError(
            'snappy_engine="device" needs the GPU engine; this write '
            f"resolved to engine={eng!r}")
    if val != "device" or codec != "snappy":
        return False
    from ..engine import gpu as gpu_engine

    block = P.snappy_block_size()
    if block > gpu_engine.SNAPPY_MAX_CHUNK_RAW:
        _log.warning(
            "snappy_engine=device: TFREC_SNAPPY_BLOCK=%d is above the "
            "device's %d bytes per chunk; compressing on the host", block,
            gpu_engine.SNAPPY_MAX_CHUNK_RAW)
        return False
    return True


def _device_image_to_pinned(img, tag: str,
                            device_codec: Optional[str]) -> np.ndarray:
    """ONE D2H of a device file image into the tag's pinned buffer. With
    `device_codec` ("gzip" or "snappy") the image is compressed in HBM
    first, so only the compressed bytes cross the host link. Returns the
    pinned view (valid until the tag's next use)."""
    from ..engine import gpu as gpu_engine

    if device_codec == "gzip":
        img = gpu_engine.gzip_image_device(img)
    elif device_codec == "snappy":
        img = gpu_engine.snappy_image_device(img)
    return gpu_engine.device_to_pinned_view(img, tag=tag)


def _encode_and_write(table: pa.Table, schema: StructType, record_type: str,
                      out_dir: str, codec: Optional[str], job_id: str,
                      num_shards: int, shard_offset: int, eng: str,
                      metrics: Optional[IOMetrics] = None,
                      device_codec: Optional[str] = None):
    """Encode `table` into `num_shards` part files under out_dir. The
    compress+write of shard k runs on a worker thread while shard k+1
    encodes (both the native encoder and zlib release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor

    R = table.num_rows
    bounds = np.linspace(0, R, num_shards + 1).astype(np.int64)

    def _compress_write(raw: bytes, fpath: str, rows: int):
        # with device_codec, `raw` already is the compressed file image
        payload = raw if device_codec else P.compress_bytes(raw, codec)
        P.write_file_atomic(payload, fpath)
        if metrics is not None:
            metrics.add(rows=rows, nbytes=len(payload), files=1)

    if num_shards == 1:
        fpath = os.path.join(out_dir, P.part_file_name(shard_offset, codec,
                                                       job_id))
        if codec is None and R > 2 * _PIPE_CHUNK_ROWS:
            # overlap convert/encode with the file append, chunk by chunk
            _single_shard_pipelined(table, schema, record_type, fpath, eng,
                                    metrics)
            return
        # no pool for a small single shard: thread spin-up dominates
        batch = table_to_batch(table, schema)
        if eng == "gpu":
            from ..engine import gpu as gpu_engine

            img = gpu_engine.encode_device(
                gpu_engine.batch_to_device(batch), record_type)
            raw = _device_image_to_pinned(img, "encw0", device_codec)
        else:
            raw = cpu_engine.encode_batch(batch, record_type)
        _compress_write(raw, fpath, R)
        return

    if R < 32_768:
        # tiny multi-shard job: pool submit/wait latency (~1 ms round trip
        # measured on the 1k-row plumbing config) dominates the actual
        # encode+write — run the shards inline
        for s in range(num_shards):
            lo, hi = int(bounds[s]), int(bounds[s + 1])
            if hi == lo:
                continue
            batch = table_to_batch(table.slice(lo, hi - lo), schema)
            if eng == "gpu":
                from ..engine import gpu as gpu_engine

                img = gpu_engine.encode_device(
                    gpu_engine.batch_to_device(batch), record_type)
                raw = _device_image_to_pinned(img, "encw0", device_codec)
            else:
                raw = cpu_engine.encode_batch(batch, record_type)
            _compress_write(raw, os.path.join(
                out_dir, P.part_file_name(shard_offset + s, codec, job_id)),
                hi - lo)
        return

    pool = P.shared_pool()
    futs = []
    tag_futs = {}
    for s in range(num_shards):
        lo, hi = int(bounds[s]), int(bounds[s + 1])
        if num_shards > 1 and hi == lo:
            continue
        chunk = table.slice(lo, hi - lo)
        batch = table_to_batch(chunk, schema)
        fname = P.part_file_name(shard_offset + s, codec, job_id)
        fpath = os.path.join(out_dir, fname)
        if eng == "gpu":
            from ..engine import gpu as gpu_engine

            # encode on device, ONE pinned D2H, write/compress on a
            # worker thread while the next shard encodes. (A mapped-DMA
            # write to the fresh temp inode pays ~0.16 ms/MB of
            # hipHostRegister each time — slower than the page-cache
            # write itself; the mapped path is for stable-inode rewrites
            # like engine-level write_batch_to_file.)
            dev_batch = gpu_engine.batch_to_device(batch)
            img = gpu_engine.encode_device(dev_batch, record_type)
            tag = f"encw{s % 2}"
            prev = tag_futs.get(tag)
            if prev is not None:
                prev.result()  # the tag's pinned buffer is being reused
            raw = _device_image_to_pinned(img, tag, device_codec)
        else:
            raw = cpu_engine.encode_batch(batch, record_type)
        f = pool.submit(_compress_write, raw, fpath, hi - lo)
        if eng == "gpu":
            tag_futs[tag] = f
        futs.append(f)
    for f in futs:
        f.result()


def write_tfrecord(data, path: str, record_type: str = "Example",
                   codec: Optional[str] = None, mode: str = "errorifexists",
                   partition_by: Optional[Sequence[str]] = None,
                   schema: Optional[StructType] = None, num_shards: int = 1,
                   engine: str = "auto", write_success: bool = True,
                   shard_offset: int = 0, job_id: Optional[str] = None,
                   _apply_mode: bool = True,
                   gzip_engine: Optional[str] = None,
                   snappy_engine: Optional[str] = None) -> None:
    """Write DataFrame-shaped `data` as TFRecord files under `path`.

    Fault tolerance: every part file lands via write-to-temp + atomic
    rename, and `_SUCCESS` is written last — a crashed job never leaves a
    partial file visible. Pass an explicit `job_id` to make retries
    idempotent: the rerun produces identical part-file names and atomically
    replaces whatever the failed attempt left behind (the analog of Spark's
    task-commit protocol the reference relies on).

    `gzip_engine`: "host" (the default; zlib on the host) or "device" (the
    GPU engine compresses gzip output in HBM and copies only the compressed
    image to the host). None takes the default, which TFREC_GZ_ENGINE sets
    for GPU-engine writes. "device" with the CPU engine is an error; with a
    codec other than gzip it is ignored.

    `snappy_engine`: the same choice for the snappy codec ("host" is
    pyarrow's Snappy, "device" the GPU engine's own compressor); the
    default comes from TFREC_SNAPPY_ENGINE for GPU-engine writes. A
    TFREC_SNAPPY_BLOCK above 1 MiB is compressed on the host either way."""
    if record_type not in RECORD_TYPES:
        raise ValueError(
            f"Unsupported recordType {record_type!r} (expected one of {RECORD_TYPES})")
    codec = P.normalize_codec(codec)
    table = normalize_input(data, schema)
    if schema is None:
        schema = schema_from_arrow(table.schema)
    validate_schema_for_record_type(schema, record_type)
    eng = engine_mod.resolve_engine(engine)
    gzip_device = _resolve_gzip_engine(gzip_engine, eng, codec)
    snappy_device = _resolve_snappy_engine(snappy_engine, eng, codec)
    # the codec the GPU engine compresses in HBM, if any
    device_codec = ("gzip" if gzip_device
                    else "snappy" if snappy_device else None)

    if record_type == "ByteArray":
        # reference: serializeByteArray frames column 0, which must be binary
        first = schema.fields[0]
        if not isinstance(first.dataType, BinaryType):
            raise TypeError(
                "ByteArray record type requires the first column to be BinaryType")

    if _apply_mode:
        if not P.apply_save_mode(path, mode):
            return
    if job_id is None:
        job_id = uuid.uuid4().hex[:12]
    metrics = IOMetrics("write")

    if partition_by:
        for c in partition_by:
            if c not in table.column_names:
                raise KeyError(f"partition column '{c}' not found")
        data_cols = [c for c in table.column_names if c not in set(partition_by)]
        data_schema = StructType([f for f in schema.fields if f.name in set(data_cols)])
        codes, combos = _factorize_partitions(table, partition_by)
        stripped = table.select(data_cols)

        def part_dir(combo) -> str:
            d = os.path.join(path, *(f"{c}={_partition_dir_value(v)}"
                                     for c, v in zip(partition_by, combo)))
            os.makedirs(d, exist_ok=True)
            return d

        if (eng == "gpu" and record_type != "ByteArray" and num_shards == 1
                and table.num_rows > 0):
            # MI355X path: encode every row ONCE on the GPU, then split into
            # per-partition file images by gathering framed records in HBM
            # (frames are concatenable — no re-serialization per partition)
            from ..engine import gpu as gpu_engine

            batch = gpu_engine.batch_to_device(
                table_to_batch(stripped, data_schema))
            img, ranges = gpu_engine.encode_partitions_device(
                batch, codes, len(combos), record_type)
            # ONE link-speed D2H of the whole partitioned image, then the
            # part files are written from pinned-view slices on a thread
            # pool (different files page-allocate concurrently; per-file
            # mmap registration would cost ~0.16 ms/MB each on the fresh
            # temp inodes — the r01 config-3 cliff)
            view = (None if device_codec
                    else gpu_engine.device_to_pinned_view(img))

            def _part_path(p):
                return os.path.join(
                    part_dir(combos[p]),
                    P.part_file_name(shard_offset, codec, job_id))

            def _write_part(p, lo, hi):
                payload = (view[lo:hi] if codec is None
                           else P.compress_bytes(view[lo:hi].tobytes(), codec))
                P.write_file_atomic(payload, _part_path(p))
                return len(payload)

            def _write_payload(payload, fpath):
                P.write_file_atomic(payload, fpath)
                return len(payload)

            # distinct partition values can share a directory (null and ""
            # both become the Hive default) and with it the part-file path:
            # write such a path once, from the last combo that maps to it —
            # what the sequential host path leaves behind — instead of
            # racing two pool threads on one rename
            owner = {}
            for p, _, _ in ranges:
                owner[tuple(_partition_dir_value(v) for v in combos[p])] = p
            ranges = [r for r in ranges if owner[tuple(
                _partition_dir_value(v) for v in combos[r[0]])] == r[0]]
            if device_codec:
                # each partition's slice of the device image compresses in
                # HBM; its write overlaps the next partition's compression
                # (two pinned buffers, as in the multi-shard path)
                pool = P.shared_pool()
                futs = []
                for k, (p, lo, hi) in enumerate(ranges):
                    if k >= 2:
                        futs[k - 2].result()  # its pinned buffer is reused
                    payload = _device_image_to_pinned(
                        img[lo:hi], f"encw{k % 2}", device_codec)
                    futs.append(pool.submit(_write_payload, payload,
                                            _part_path(p)))
                sizes = [f.result() for f in futs]
            else:
                sizes = P.shared_pool().map(lambda a: _write_part(*a), ranges)
            for nb in sizes:
                if metrics is not None:
                    metrics.add(nbytes=nb, files=1)
            if metrics is not None:
                metrics.add(rows=table.num_rows)
        else:
            for p, combo in enumerate(combos):
                idxs = np.nonzero(codes == p)[0]
                if idxs.size == 0:
                    continue
                sub = stripped.take(pa.array(idxs, type=pa.int64()))
                _encode_and_write(sub, data_schema, record_type, part_dir(combo),
                                  codec, job_id, num_shards, shard_offset, eng,
                                  metrics, device_codec)
    else:
        _encode_and_write(table, schema, record_type, path, codec, job_id,
                          num_shards, shard_offset, eng, metrics, device_codec)

    if write_success:
        P.write_success_marker(path)
    metrics.finish()
