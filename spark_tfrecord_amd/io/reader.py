"""Read path: TFRecord files -> DataFrame.

Mirrors the reference's read pipeline: file discovery
(whole files, never split — gzip streams can't be, DefaultSource.scala:26-29),
schema inference from the first non-empty file when no schema is given,
per-file decode, and partition-column discovery from `col=value/` directory
names (the part Spark's planner did above the reference library).
"""

from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import pyarrow as pa

from .. import engine as engine_mod
from ..arrow_interop import batch_to_table, schema_to_arrow
from ..engine import cpu as cpu_engine
from ..infer import (
    byte_array_schema,
    infer_codes_from_buffer,
    merge_code_maps,
    schema_from_codes,
)
from ..schema import (LongType, StringType, StructField, StructType,
                      validate_schema_for_record_type)
from ..utils import IOMetrics, StageTimer
from .. import _native
from . import paths as P

__all__ = ["read_tfrecord", "infer_schema_of_paths"]

FOREIGN_GZIP_MODES = ("host", "device")


def _resolve_foreign_gzip(foreign_gzip: Optional[str], eng: str) -> bool:
    """True when gzip files WITHOUT our segment table (any other writer's)
    are inflated in HBM by the speculative inflater
    (csrc/hip/inflate_foreign.hip) instead of by host zlib. None = the
    default: "host", or what TFREC_GZ_FOREIGN says for GPU-engine reads."""
    explicit = foreign_gzip is not None
    if not explicit:
        foreign_gzip = (os.environ.get("TFREC_GZ_FOREIGN", "host")
                        if eng == "gpu" else "host")
    val = str(foreign_gzip).lower()
    if val not in FOREIGN_GZIP_MODES:
        raise ValueError(
            f"Unsupported foreign gzip mode {foreign_gzip!r} (expected one "
            f"of {FOREIGN_GZIP_MODES})")
    if val == "device" and eng != "gpu":
        raise ValueError(
            'foreign_gzip="device" needs the GPU engine; this read resolved '
            f"to engine={eng!r}")
    return val == "device"


def _load_file(path: str) -> np.ndarray:
    return np.frombuffer(P.decompress_file(path), np.uint8)


def _scanned_files(files: List[str], eng: str):
    """(image, frame offsets, frame lengths) of each non-empty file, in
    order: device tensors where the GPU engine takes the file
    (gpu.device_source, foreign gzip left to the host), numpy arrays of the
    host codec's bytes otherwise."""
    for f in files:
        if eng == "gpu" and os.path.getsize(f):
            from ..engine import gpu as gpu_engine

            data = gpu_engine.read_file_image(f)
            if data is not None:
                if data.numel():
                    yield (data, *gpu_engine.scan_frames_device(data))
                continue
        data = _load_file(f)
        if data.size:
            yield (data, *_native.scan_frames(data, False))


def infer_schema_of_paths(files: List[str], record_type: str,
                          engine: str = "cpu") -> StructType:
    """Schema from the FIRST non-empty file (DefaultSource.scala:36-38
    collectFirst), scanned fully — on the GPU (hash-table lattice kernel)
    when engine='gpu' and the device takes the file."""
    if record_type == "ByteArray":
        return byte_array_schema()
    for data, off, lens in _scanned_files(files, engine):
        if len(off) == 0:
            continue
        if isinstance(data, np.ndarray):
            codes = infer_codes_from_buffer(data, off, lens, record_type)
        else:
            from ..engine import gpu as gpu_engine

            codes = gpu_engine.infer_codes_device(data, off, lens, record_type)
        return schema_from_codes(codes) if codes else StructType([])
    raise ValueError("Could not infer schema: no non-empty TFRecord files found")


def _partition_schema(files: List[str], base_dir: str) -> List[str]:
    cols: List[str] = []
    for f in files:
        for k in P.partition_values_of(f, base_dir):
            if k not in cols:
                cols.append(k)
    return cols


def _partition_col_array(values: List[str], n: int):
    """Spark-style partition value type inference: int64 if all parse, else
    string."""
    try:
        return pa.array([int(v) for v in values], type=pa.int64())
    except (ValueError, TypeError):
        return pa.array(
            [None if v == "__HIVE_DEFAULT_PARTITION__" else v for v in values],
            type=pa.large_utf8())


def count_tfrecord(path: str, engine: str = "auto") -> int:
    """Total record count without decoding any payloads (frame scan only —
    the GPU path discovers and chains frame boundaries in parallel)."""
    files = P.list_data_files(path)
    if not files:
        raise FileNotFoundError(f"No TFRecord files found under {path}")
    eng = engine_mod.resolve_engine(engine)
    return sum(len(off) for _, off, _ in _scanned_files(files, eng))


def read_tfrecord(path: str, schema: Optional[StructType] = None,
                  record_type: str = "Example", engine: str = "auto",
                  verify_crc: bool = True, base_dir: Optional[str] = None,
                  columns: Optional[List[str]] = None,
                  foreign_gzip: Optional[str] = None):
    """Read a TFRecord dataset as a DataFrame.

    `foreign_gzip` "device" inflates gzip files that other programs wrote
    (no segment table) on the GPU, "host" (the default, or TFREC_GZ_FOREIGN)
    leaves them to host zlib; a file the device refuses is read on the host
    either way.

    `columns` projects the read: only the named fields are scanned and
    extracted (the schema-driven kernels skip other features entirely, like
    the reference's deserializer ignores unknown ones)."""
    from ..api import DataFrame

    if record_type not in ("Example", "SequenceExample", "ByteArray"):
        raise ValueError(f"Unsupported recordType {record_type!r}")
    files = P.list_data_files(path)
    if not files:
        raise FileNotFoundError(f"No TFRecord files found under {path}")
    if base_dir is None:
        if isinstance(path, (list, tuple)):
            base_dir = (os.path.commonpath([os.path.dirname(f) for f in files])
                        if files else "")
        else:
            base_dir = path if os.path.isdir(path) else os.path.dirname(path)
    part_cols = _partition_schema(files, base_dir) if base_dir else []
    eng = engine_mod.resolve_engine(engine)
    foreign_device = _resolve_foreign_gzip(foreign_gzip, eng)
    if eng == "gpu":
        from ..engine import gpu as gpu_engine

    metrics = IOMetrics("read")

    # Files needing host bytes (compressed, or CPU engine) are loaded and
    # inflated by a thread pool — gzip/zlib release the GIL, so multi-file
    # reads decompress in parallel (gzip itself is sequential PER file,
    # matching the reference's isSplitable=false model). A sliding window
    # bounds resident decompressed bytes.
    from concurrent.futures import ThreadPoolExecutor

    # path -> gpu.device_source record, None = host bytes; each file is
    # classified once per read (its header or block table walked once), and
    # a file the device then refuses is set to None
    sources: dict = {}

    def _source(fpath: str):
        if fpath not in sources:
            sources[fpath] = (gpu_engine.device_source(fpath, foreign_device)
                              if eng == "gpu" else None)
        return sources[fpath]

    # Schema-less GPU reads DEFER inference into the first group pipeline:
    # the file image is scanned once in HBM, the lattice kernel runs over
    # the first non-empty file's frames, and the decode reuses the image —
    # one pass instead of the reference's extra inference job.
    deferred_infer = (schema is None and eng == "gpu" and bool(files)
                      and _source(files[0]) is not None)
    if schema is None and not deferred_infer:
        with StageTimer(metrics, "infer_schema"):
            schema = infer_schema_of_paths(files, record_type, eng)

    def _resolve(schema):
        nonlocal part_cols
        if columns is not None:
            missing = [c for c in columns
                       if c not in [f.name for f in schema.fields]
                       and c not in part_cols]
            if missing:
                raise KeyError(f"columns not in schema: {missing}")
            schema = StructType(
                [f for f in schema.fields if f.name in set(columns)])
            part_cols = [c for c in part_cols if c in set(columns)]
        data_schema = StructType(
            [f for f in schema.fields if f.name not in part_cols])
        # an Example cannot carry 2-D ragged fields: reject like the
        # reference's deserializer would (TFRecordDeserializer.scala:148-175)
        validate_schema_for_record_type(data_schema, record_type)
        return data_schema

    data_schema = None if deferred_infer else _resolve(schema)

    workers = min(32, (os.cpu_count() or 8))
    window = 2 * workers
    futures: dict = {}
    _pool = P.shared_pool  # persistent process-wide pool (no spin-up)

    def _host_task(fpath: str):
        data = _load_file(fpath)
        if data.size == 0 or eng == "gpu":
            return data  # GPU engine decodes on the device stream
        # the native codec releases the GIL: files decode concurrently
        return cpu_engine.decode_buffer(data, data_schema, record_type,
                                        verify_crc=verify_crc)

    # tiny jobs (<= 2 small files) skip the pool: submit/wait latency
    # dominates sub-ms decodes (the 1k-row plumbing config round trip)
    _inline_small = (len(files) <= 2 and
                     all(os.path.getsize(f) < (256 << 10) for f in files))

    def _blob(i: int):
        f = futures.pop(i, None)
        if f is not None:
            return f.result()
        if _inline_small:
            return _host_task(files[i])
        return _pool().submit(_host_task, files[i]).result()

    # GPU path: consecutive uncompressed files are decoded as ONE pipeline
    # (images concatenated in HBM — frames are concatenable — scanned and
    # decoded in a single pass, rows split per file afterwards). Compressed
    # files and the CPU engine go file-by-file through host bytes.
    _GROUP_BYTES = 4 << 30

    def _read_group(group, schema):
        """One pipeline over the group's files; schema None = infer it from
        the group's first non-empty file on the way."""
        return gpu_engine.read_files_to_batch(
            group, schema, record_type, verify_crc=verify_crc,
            foreign_gzip=foreign_device, sources=[sources[f] for f in group])

    def _infer_from_files():
        """The fallback where no group could infer: from the whole list."""
        return _resolve(infer_schema_of_paths(files, record_type, eng))

    def _append_with_parts(t, fpaths, row_counts):
        pvs = [P.partition_values_of(f, base_dir) for f in fpaths]
        for c in part_cols:
            vals = np.repeat([pv.get(c) for pv in pvs], row_counts).tolist()
            t = t.append_column(c, _partition_col_array(vals, t.num_rows))
        tables.append(t)

    tables = []
    try:
        i = 0
        while i < len(files):
            fpath = files[i]
            if _source(fpath) is not None:
                group = []
                gbytes = 0
                i0 = i
                while (i < len(files) and _source(files[i]) is not None
                       and gbytes < _GROUP_BYTES):
                    group.append(files[i])
                    gbytes += os.path.getsize(files[i])
                    i += 1
                try:
                    if data_schema is None:
                        try:
                            batch, row_counts = _read_group(group, None)
                            data_schema = _resolve(batch.schema)
                        except ValueError:
                            # this group was entirely empty: resolve the
                            # schema from the full file list, then decode
                            # normally
                            data_schema = _infer_from_files()
                            batch, row_counts = _read_group(group, data_schema)
                    else:
                        batch, row_counts = _read_group(group, data_schema)
                except gpu_engine.DeviceDecompressRejected as rej:
                    # redo the group without the refused files: they take
                    # the host path, as with foreign_gzip="host" (gzip) or
                    # TFREC_SNAPPY=host (snappy)
                    import logging

                    for p in rej.paths:
                        sources[p] = None  # host bytes from here on
                        if isinstance(rej, gpu_engine.ForeignGzipRejected):
                            logging.getLogger(__name__).warning(
                                "device inflate refused foreign gzip file "
                                "%s; host zlib fallback", p)
                        else:
                            logging.getLogger(__name__).warning(
                                "device decode refused %s; host codec "
                                "fallback", p)
                    i = i0
                    continue
                for f in group:
                    metrics.add(files=1, nbytes=os.path.getsize(f))
                if batch.num_rows == 0 and not part_cols:
                    continue
                t = batch_to_table(gpu_engine.batch_to_host(batch))
                if [f.name for f in data_schema.fields] != t.column_names:
                    # deferred inference + column projection: decode carried
                    # the full inferred schema; project here
                    t = t.select([f.name for f in data_schema.fields])
                _append_with_parts(t, group, row_counts)
                continue
            for j in range(i, min(i + window, len(files))):
                if (not _inline_small and _source(files[j]) is None
                        and j not in futures):
                    futures[j] = _pool().submit(_host_task, files[j])
            metrics.add(files=1, nbytes=os.path.getsize(fpath))
            if data_schema is None:
                # inference was deferred to a group the device then refused
                with StageTimer(metrics, "infer_schema"):
                    data_schema = _infer_from_files()
            got = _blob(i)
            i += 1
            if eng == "gpu":
                if got.size == 0:
                    continue
                batch = gpu_engine.decode_buffer_to_cpu(
                    got, data_schema, record_type, verify_crc=verify_crc)
            else:
                if isinstance(got, np.ndarray):  # empty file sentinel
                    continue
                batch = got
            t = batch_to_table(batch)
            _append_with_parts(t, [fpath], [t.num_rows])
    finally:
        for f in futures.values():  # abandon prefetches from a failed read
            f.cancel()
    if not tables:
        full = StructType(list(data_schema.fields) +
                          [StructField(c, StringType(), True) for c in part_cols])
        empty = pa.table({f.name: [] for f in full.fields},
                         schema=schema_to_arrow(full))
        return DataFrame(empty, full)

    # Partition column types must agree across files: rebuild as common type
    table = pa.concat_tables(tables, promote_options="permissive")
    full_schema = StructType(list(data_schema.fields))
    for c in part_cols:
        at = table.schema.field(c).type
        full_schema.add(c, LongType() if pa.types.is_integer(at) else StringType())
    metrics.add(rows=table.num_rows)
    metrics.finish()
    return DataFrame(table, full_schema)
