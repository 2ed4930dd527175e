#!/usr/bin/env python3
"""Benchmark suite for the non-flagship BASELINE.json configs.

bench.py measures config 2 (the headline 1M-row Example round-trip; the
driver runs it). This suite covers the rest, each printing one JSON line:

  plumbing        config 1: 1k-row scalar Example round-trip, CPU engine
                  (the reference's Spark local[2] analog; 2 shards)
  partitionby     config 3: Example partitionBy("date") write; with
                  WORLD_SIZE>1 the rows are exchanged with the RCCL
                  all-to-all so each date has one writer rank
  infer           config 4: SequenceExample (FeatureList of FloatList)
                  schema inference; with WORLD_SIZE>1 the per-feature
                  lattice codes are max-all-reduced over RCCL
  gzip_write      GPU-engine gzip write, host zlib vs the device compressor
                  (gzip_engine="host" | "device"), on flagship-shaped
                  Example rows and on config 5's random ByteArray payloads
  gzip_foreign    GPU-engine read of gzip files another program wrote (zlib
                  level 6, no segment table): host zlib pool vs the
                  speculative device inflater (foreign_gzip="host" |
                  "device"), as one file and as 32 files
  snappy_write    GPU-engine snappy write of flagship rows, pyarrow's Snappy
                  on the host vs the device compressor (snappy_engine="host"
                  | "device"), as 1 shard and as 8 shards
  gzip_bytearray  config 5: gzip-compressed ByteArray read, shard staged
                  through HBM on the GPU engine
  collate         dense training batches of 8192 flagship rows from 8
                  shards: TFRecordIterableDataset (ragged wire form) against
                  TFRecordBatchDataset (collate kernel) without and with a
                  shuffle window, and the kernel against the same collation
                  in torch indexing ops on one decoded shard

Single process:  python bench_suite.py all --rows 100000
Multi GPU:       torchrun --nproc-per-node 8 bench_suite.py partitionby
"""

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _env_world():
    return (int(os.environ.get("RANK", "0")),
            int(os.environ.get("WORLD_SIZE", "1")))


def _emit(rank, metric, value, unit, config, elapsed, n_gpus):
    if rank == 0:
        print(json.dumps({
            "metric": metric, "value": value, "unit": unit,
            "n_gpus": n_gpus, "elapsed_s": round(elapsed, 4),
            "higher_is_better": True, "data": "synthetic", "config": config,
        }), flush=True)


def _workdir(tag, rank):
    base = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    d = os.path.join(base, f"tfrec_suite_{tag}_r{rank}")
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d, exist_ok=True)
    return d


def bench_plumbing(args):
    """Config 1: 1k-row scalar-only DataFrame round-trip on CPU, 2 shards."""
    import spark_tfrecord_amd as stf

    rng = np.random.default_rng(0)
    n = 1000
    data = {"lng": rng.integers(0, 2**40, n),
            "flt": rng.random(n).astype(np.float32),
            "s": [f"row-{i}" for i in range(n)]}
    d = _workdir("plumbing", 0)
    out = os.path.join(d, "t")
    reps = args.reps
    # one untimed warmup round-trip (module/thread-pool/arrow first-call costs)
    stf.write_tfrecord(data, out, engine="cpu", mode="overwrite", num_shards=2)
    stf.read_tfrecord(out, engine="cpu")
    t0 = time.perf_counter()
    for r in range(reps):
        stf.write_tfrecord(data, out, engine="cpu", mode="overwrite",
                           num_shards=2)
        df = stf.read_tfrecord(out, engine="cpu")
        assert df.count() == n
    el = time.perf_counter() - t0
    _emit(0, "rows/sec round-trip (1k-row scalar CPU plumbing)",
          n * reps / el, "rows/s",
          {"rows": n, "shards": 2, "engine": "cpu", "reps": reps}, el, 0)


def bench_partitionby(args):
    """Config 3: partitionBy("date") write; all-to-all shuffle when world>1."""
    import torch

    from spark_tfrecord_amd.parallel import dist as D

    rank, world = _env_world()
    use_cuda = torch.cuda.is_available()
    if world > 1:
        D.init_distributed()
    import pyarrow as pa

    rows = args.rows // world
    rng = np.random.default_rng(100 + rank)
    # build the arrow table ONCE: the timed loop measures the engine, not
    # python->arrow input conversion
    data = pa.table({
        "date": pa.array([f"2026-09-{d:02d}" for d in
                          rng.integers(1, 11, rows)]),
        "uid": pa.array(rng.integers(0, 2**62, rows)),
        "score": pa.array(rng.random(rows).astype(np.float32)),
        "feats": pa.array(list(rng.random((rows, 8)).astype(np.float32))),
    })
    # shared dir: ranks write distinct part files; rank 0 alone prepares it
    if world == 1 or rank == 0:
        d = _workdir("partby", 0)
    else:
        base = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
        d = os.path.join(base, "tfrec_suite_partby_r0")
    out = os.path.join(d, "t")
    eng = "gpu" if use_cuda else "cpu"

    def sync():
        if use_cuda:
            torch.cuda.synchronize()
        if world > 1:
            import torch.distributed as td
            td.barrier()

    sync()  # setup rmtree (rank 0) must complete before anyone writes

    def one_rep():
        if world > 1:
            D.write_tfrecord_distributed(data, out, partition_by=["date"],
                                         mode="overwrite", engine=eng)
        else:
            import spark_tfrecord_amd as stf
            stf.write_tfrecord(data, out, partition_by=["date"],
                               mode="overwrite", engine=eng)

    one_rep()  # untimed warmup
    sync()
    t0 = time.perf_counter()
    for r in range(args.reps):
        one_rep()
    sync()
    el = time.perf_counter() - t0
    total = rows * world * args.reps
    _emit(rank, "rows/sec partitionBy write (all-to-all shuffle)",
          total / el, "rows/s",
          {"rows_total": rows * world, "partitions": 10, "engine": eng,
           "parallelism": f"dp{world}", "reps": args.reps}, el,
          world if use_cuda else 0)


def bench_infer(args):
    """Config 4: SequenceExample schema inference (+ all-reduce when world>1)."""
    import torch

    import spark_tfrecord_amd as stf
    from spark_tfrecord_amd.io.reader import infer_schema_of_paths
    from spark_tfrecord_amd.parallel import dist as D

    rank, world = _env_world()
    use_cuda = torch.cuda.is_available()
    if world > 1:
        D.init_distributed()

    def sync():
        if use_cuda:
            torch.cuda.synchronize()
        if world > 1:
            import torch.distributed as td
            td.barrier()

    # ONE shared dataset (the distributed contract: every rank passes the
    # SAME file list; rank r scans records r::world of the chosen file and
    # the lattice codes are max-all-reduced)
    rows = args.rows
    d = _workdir("infer", 0) if (world == 1 or rank == 0) else None
    if d is None:
        base = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
        d = os.path.join(base, "tfrec_suite_infer_r0")
    out = os.path.join(d, "t")
    if rank == 0:
        rng = np.random.default_rng(7)
        # ragged 2-D: FeatureList of FloatList
        rag = [[list(rng.random(rng.integers(1, 6)).astype(float))
                for _ in range(int(rng.integers(1, 5)))] for _ in range(rows)]
        data = {"sid": np.arange(rows, dtype=np.int64), "rag": rag}
        schema = stf.StructType([
            stf.StructField("sid", stf.LongType(), True),
            stf.StructField("rag",
                            stf.ArrayType(stf.ArrayType(stf.FloatType())), True),
        ])
        stf.write_tfrecord(data, out, record_type="SequenceExample",
                           schema=schema,
                           engine="gpu" if use_cuda else "cpu",
                           mode="overwrite")
    sync()
    files = [os.path.join(out, f) for f in sorted(os.listdir(out))
             if not f.startswith("_")]

    def one_rep():
        if world > 1:
            return D.infer_schema_distributed(files, "SequenceExample")
        return infer_schema_of_paths(files, "SequenceExample",
                                     "gpu" if use_cuda else "cpu")

    s = one_rep()  # untimed warmup
    sync()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        s = one_rep()
    sync()
    el = time.perf_counter() - t0
    assert "rag" in [f.name for f in s.fields]
    total = rows * args.reps  # shared file: `rows` records scanned per rep
    _emit(rank, "records/sec schema inference (SequenceExample lattice)",
          total / el, "records/s",
          {"rows_total": rows, "parallelism": f"dp{world}",
           "engine": "gpu" if use_cuda else "cpu", "reps": args.reps}, el,
          world if use_cuda else 0)


def bench_gzip_bytearray(args):
    """Config 5: gzip ByteArray read, shard staged through HBM."""
    import torch

    import spark_tfrecord_amd as stf

    from spark_tfrecord_amd.parallel import dist as D

    rank, world = _env_world()
    use_cuda = torch.cuda.is_available()
    if world > 1:
        D.init_distributed()

    def sync():
        if use_cuda:
            torch.cuda.synchronize()
        if world > 1:
            import torch.distributed as td
            td.barrier()

    rows = args.rows // max(world, 1)
    rng = np.random.default_rng(9 + rank)
    payloads = [rng.bytes(200) for _ in range(rows)]
    import pyarrow as pa
    table = pa.table({"byteArray": pa.array(payloads, type=pa.large_binary())})
    d = _workdir("gzba", rank)
    out = os.path.join(d, "t")
    # many shards, like one Spark task per file in the reference: gzip is
    # sequential PER file, so shards are the parallelism axis on read
    stf.write_tfrecord(table, out, record_type="ByteArray", codec="gzip",
                       mode="overwrite", engine="cpu", num_shards=32)
    nbytes = sum(os.path.getsize(os.path.join(out, f))
                 for f in os.listdir(out) if not f.startswith("_"))
    eng = "gpu" if use_cuda else "cpu"
    stf.read_tfrecord(out, record_type="ByteArray", engine=eng)  # warmup
    sync()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        df = stf.read_tfrecord(out, record_type="ByteArray", engine=eng)
        assert df.count() == rows
    sync()
    el = time.perf_counter() - t0
    _emit(rank, "rows/sec gzip ByteArray read",
          rows * world * args.reps / el, "rows/s",
          {"rows_total": rows * world, "gz_bytes_per_rank": nbytes,
           "engine": eng, "parallelism": f"dp{world}", "reps": args.reps}, el,
          world if use_cuda else 0)


def _flagship_table(rows, seed):
    """bench.py's Example shape as an Arrow table: int64 id, Int64List[8],
    FloatList[16], BytesList[2] of ~12-byte tokens (~220 B/record)."""
    import pyarrow as pa

    rng = np.random.default_rng(seed)

    def lists(values, k):
        return pa.ListArray.from_arrays(
            pa.array(np.arange(0, (rows + 1) * k, k, dtype=np.int32)), values)

    toks = [f"tok{i % 997:06d}-{i % 89:02d}" for i in range(2 * rows)]
    return pa.table({
        "id": pa.array(rng.integers(0, 2**62, rows).astype(np.int64)),
        "ints": lists(pa.array(
            rng.integers(0, 2**31, 8 * rows).astype(np.int64)), 8),
        "floats": lists(pa.array(rng.random(16 * rows).astype(np.float32)), 16),
        "tokens": lists(pa.array(toks, type=pa.string()), 2),
    })


def bench_gzip_write(args):
    """GPU-engine gzip write: host zlib (the default) against the device
    DEFLATE compressor, same build, same data. Two datasets: Example rows
    (feature names repeat every record: match-heavy) and config 5's random
    200-byte ByteArray payloads (incompressible: the stored path)."""
    import pyarrow as pa
    import torch

    import spark_tfrecord_amd as stf

    rank, world = _env_world()
    if not torch.cuda.is_available():
        raise SystemExit("gzip_write needs the GPU engine")
    rows = args.rows // max(world, 1)
    rng = np.random.default_rng(9 + rank)
    datasets = [
        ("example", "Example", _flagship_table(rows, 1 + rank)),
        ("bytearray", "ByteArray", pa.table({"byteArray": pa.array(
            [rng.bytes(200) for _ in range(rows)], type=pa.large_binary())})),
    ]
    d = _workdir("gzw", rank)
    for name, rtype, table in datasets:
        for gz in ("host", "device"):
            out = os.path.join(d, f"{name}_{gz}")

            def write():
                stf.write_tfrecord(table, out, record_type=rtype, codec="gzip",
                                   mode="overwrite", engine="gpu",
                                   gzip_engine=gz)
                torch.cuda.synchronize()

            write()  # warm-up: allocator pools, pinned buffers, page cache
            t0 = time.perf_counter()
            for _ in range(args.reps):
                write()
            el = time.perf_counter() - t0
            nbytes = sum(os.path.getsize(os.path.join(out, f))
                         for f in os.listdir(out) if not f.startswith("_"))
            _emit(rank, f"rows/sec gzip write {name} gzip_engine={gz}",
                  rows * args.reps / el, "rows/s",
                  {"rows": rows, "dataset": name, "gzip_engine": gz,
                   "gz_bytes": nbytes, "engine": "gpu", "reps": args.reps},
                  el, 1)
    shutil.rmtree(d, ignore_errors=True)


def bench_gzip_foreign(args):
    """GPU-engine read of foreign gzip (flagship-shaped Example frames
    recompressed by zlib level 6 into plain gzip members): foreign_gzip=
    "host" against "device", alternating in one process after a warm-up.
    One file of --rows rows is single-stream latency; 32 files of --rows/32
    are aggregate throughput."""
    import zlib

    import torch

    import spark_tfrecord_amd as stf
    from spark_tfrecord_amd.engine import gpu as gpu_engine
    from spark_tfrecord_amd.io import paths as P

    rank, world = _env_world()
    if not torch.cuda.is_available():
        raise SystemExit("gzip_foreign needs the GPU engine")
    d = _workdir("gzf", rank)
    for nfiles in (1, 32):
        rows = max(args.rows // nfiles, 1) * nfiles
        src = os.path.join(d, f"src{nfiles}")
        stf.write_tfrecord(_flagship_table(rows, 3 + rank), src,
                           record_type="Example", num_shards=nfiles,
                           engine="gpu")
        out = os.path.join(d, f"foreign{nfiles}")
        os.makedirs(out)
        raw_bytes = gz_bytes = 0
        for k, f in enumerate(P.list_data_files(src)):
            with open(f, "rb") as fh:
                raw = fh.read()
            co = zlib.compressobj(6, zlib.DEFLATED, 31)  # gzip wrapper
            blob = co.compress(raw) + co.flush()
            with open(os.path.join(out, f"part-{k:05d}.tfrecord.gz"),
                      "wb") as fh:
                fh.write(blob)
            raw_bytes += len(raw)
            gz_bytes += len(blob)
        schema = stf.read_tfrecord(src, engine="gpu").schema
        shutil.rmtree(src, ignore_errors=True)

        def read(mode):
            df = stf.read_tfrecord(out, schema=schema, engine="gpu",
                                   foreign_gzip=mode)
            torch.cuda.synchronize()
            return df

        el = {"host": 0.0, "device": 0.0}
        live = []
        for mode in el:
            assert read(mode).count() == rows  # warm-up
        for _ in range(args.reps):
            for mode in el:
                t0 = time.perf_counter()
                read(mode)
                el[mode] += time.perf_counter() - t0
                if mode == "device":
                    live = [e[1] for e in gpu_engine.last_foreign]
        for mode, t in el.items():
            dev = mode == "device"
            _emit(rank, f"rows/sec foreign gzip read files={nfiles} "
                        f"foreign_gzip={mode}",
                  rows * args.reps / t, "rows/s",
                  {"rows": rows, "files": nfiles, "foreign_gzip": mode,
                   "raw_gb_per_s": round(raw_bytes * args.reps / t / 1e9, 4),
                   "gz_bytes": gz_bytes, "raw_bytes": raw_bytes,
                   # bytes over the host link per read: the compressed
                   # files (device) or the inflated images (host) go up;
                   # the decoded columns come down either way
                   "h2d_bytes": gz_bytes if dev else raw_bytes,
                   "live_chunks_per_file": (
                       round(float(np.mean(live)), 1) if dev and live
                       else None),
                   "device_over_host": round(el["host"] / el["device"], 3),
                   "engine": "gpu", "reps": args.reps}, t, 1)
    shutil.rmtree(d, ignore_errors=True)


def bench_snappy(args):
    """GPU-engine read of --rows flagship Example rows written once with
    codec="snappy" (8 shards): the device Snappy decoder against
    TFREC_SNAPPY=host (pyarrow on the host), and against the same rows as
    own-format gzip through the device inflater. The three alternate in one
    process after a warm-up."""
    import torch

    import spark_tfrecord_amd as stf
    from spark_tfrecord_amd.engine import gpu as gpu_engine
    from spark_tfrecord_amd.io import paths as P

    rank, world = _env_world()
    if not torch.cuda.is_available():
        raise SystemExit("snappy needs the GPU engine")
    rows = args.rows
    d = _workdir("snp", rank)
    table = _flagship_table(rows, 5 + rank)
    dirs = {}
    sizes = {}
    for codec in ("snappy", "gzip"):
        dirs[codec] = os.path.join(d, codec)
        stf.write_tfrecord(table, dirs[codec], record_type="Example",
                           codec=codec, num_shards=8, engine="gpu")
        sizes[codec] = sum(os.path.getsize(f)
                           for f in P.list_data_files(dirs[codec]))
    schema = stf.read_tfrecord(dirs["snappy"], engine="gpu").schema
    del table
    modes = {"snappy device": ("snappy", "device"),
             "snappy host": ("snappy", "host"),
             "gzip device": ("gzip", "device")}

    def read(mode):
        codec, knob = modes[mode]
        os.environ["TFREC_SNAPPY"] = knob
        del gpu_engine.last_snappy[:]
        df = stf.read_tfrecord(dirs[codec], schema=schema, engine="gpu")
        torch.cuda.synchronize()
        assert bool(gpu_engine.last_snappy) == (mode == "snappy device")
        return df

    el = dict.fromkeys(modes, 0.0)
    chunks = 0
    for mode in modes:
        assert read(mode).count() == rows  # warm-up
    for _ in range(args.reps):
        for mode in modes:
            t0 = time.perf_counter()
            read(mode)
            el[mode] += time.perf_counter() - t0
            if mode == "snappy device":
                chunks = sum(e[1] for e in gpu_engine.last_snappy)
    os.environ.pop("TFREC_SNAPPY", None)
    for mode, t in el.items():
        codec = modes[mode][0]
        _emit(rank, f"rows/sec read {mode}", rows * args.reps / t, "rows/s",
              {"rows": rows, "files": 8, "mode": mode,
               "file_bytes": sizes[codec],
               "snappy_over_gzip_bytes": round(
                   sizes["snappy"] / sizes["gzip"], 3),
               "snappy_chunks": chunks if mode == "snappy device" else None,
               "device_over_host": round(
                   el["snappy host"] / el["snappy device"], 3),
               "device_snappy_over_device_gzip": round(
                   el["gzip device"] / el["snappy device"], 3),
               "engine": "gpu", "reps": args.reps}, t, 1)
    shutil.rmtree(d, ignore_errors=True)


def bench_snappy_write(args):
    """GPU-engine snappy write of --rows flagship Example rows: pyarrow's
    Snappy on the host (the default) against the device compressor, same
    build, same data, as 1 shard and as 8 shards. The two engines alternate
    in one process after a warm-up of each."""
    import torch

    import spark_tfrecord_amd as stf
    from spark_tfrecord_amd.io import paths as P

    rank, world = _env_world()
    if not torch.cuda.is_available():
        raise SystemExit("snappy_write needs the GPU engine")
    rows = args.rows // max(world, 1)
    table = _flagship_table(rows, 7 + rank)
    d = _workdir("snw", rank)
    engines = ("host", "device")
    for shards in (1, 8):
        outs = {e: os.path.join(d, f"s{shards}_{e}") for e in engines}

        def write(e):
            stf.write_tfrecord(table, outs[e], record_type="Example",
                               codec="snappy", mode="overwrite", engine="gpu",
                               num_shards=shards, snappy_engine=e)
            torch.cuda.synchronize()

        el = dict.fromkeys(engines, 0.0)
        for e in engines:
            write(e)  # warm-up: allocator pools, pinned buffers, page cache
        for _ in range(args.reps):
            for e in engines:
                t0 = time.perf_counter()
                write(e)
                el[e] += time.perf_counter() - t0
        sizes = {e: sum(os.path.getsize(f) for f in P.list_data_files(outs[e]))
                 for e in engines}
        got = stf.read_tfrecord(outs["device"], engine="gpu").count()
        assert got == rows, (got, rows)
        for e in engines:
            _emit(rank, f"rows/sec snappy write {shards} shard(s) "
                        f"snappy_engine={e}",
                  rows * args.reps / el[e], "rows/s",
                  {"rows": rows, "shards": shards, "snappy_engine": e,
                   "snappy_bytes": sizes[e],
                   "device_over_host": round(el["host"] / el["device"], 3),
                   "device_over_host_bytes": round(
                       sizes["device"] / sizes["host"], 4),
                   "engine": "gpu", "reps": args.reps}, el[e], 1)
    shutil.rmtree(d, ignore_errors=True)


def _torch_collate(batch, lo, hi, torch):
    """The flagship spec (id FixedLen(), ints Padded(8), floats FixedLen(16),
    tokens Padded2D(2, 12)) for rows [lo, hi) of one decoded shard in torch
    indexing ops only, with no host wait: the comparison for
    collate_rows_kernel. General in the counts (it reads the offsets), as the
    kernel is; the error flag stays on the device."""
    idc, ints, floats, tokens = (batch.column(n) for n in
                                 ("id", "ints", "floats", "tokens"))
    dev = idc.values.device

    def padded(col, L, pad):
        start = col.row_off[lo:hi]
        cnt = col.row_off[lo + 1:hi + 1] - start
        j = torch.arange(L, device=dev)
        idx = (start[:, None] + j).clamp_(max=col.values.numel() - 1)
        v = torch.where(j < cnt[:, None], col.values[idx], pad)
        return v, cnt

    out = {}
    v, cnt = padded(idc, 1, 0)
    out["id"] = v[:, 0]
    bad = (cnt != 1).any()
    out["ints"], cnt = padded(ints, 8, 0)
    out["ints_len"] = cnt.clamp(max=8).int()
    bad = bad | (cnt > 8).any()
    out["floats"], cnt = padded(floats, 16, 0.0)
    bad = bad | (cnt != 16).any()
    T, L = 2, 12
    start = tokens.row_off[lo:hi]
    oc = tokens.row_off[lo + 1:hi + 1] - start
    t = torch.arange(T, device=dev)
    item = (start[:, None] + t).clamp_(max=tokens.elem_off.numel() - 2)
    b0 = tokens.elem_off[item]
    ln = torch.where(t < oc[:, None], tokens.elem_off[item + 1] - b0, 0)
    j = torch.arange(L, device=dev)
    idx = (b0[..., None] + j).clamp_(max=tokens.values.numel() - 1)
    out["tokens"] = torch.where(j < ln[..., None], tokens.values[idx], 0)
    out["tokens_outer"] = oc.clamp(max=T).int()
    out["tokens_len"] = ln.clamp(max=L).int()
    out["_bad"] = bad | (oc > T).any() | (ln > L).any()
    return out


def bench_collate(args):
    """--rows flagship Example rows in 8 shards, batches of 8192. Whole
    pipelines, alternating after a warm-up of each: (a) the ragged
    TFRecordIterableDataset, (b) TFRecordBatchDataset with shuffle_window=0,
    (c) the same with shuffle_window=4, (c4) that with prefetch=4. Collation
    alone over one decoded
    shard: (k) collate_rows_kernel through Collator.run, (d) the same four
    columns in torch indexing ops. --collate-part kernel|torch runs only
    (k) or (d), for a kernel trace of its own; none only decodes the shard."""
    import torch

    import spark_tfrecord_amd as stf
    from spark_tfrecord_amd.collate import Collator
    from spark_tfrecord_amd.engine import gpu as gpu_engine
    from spark_tfrecord_amd.io import paths as P
    from spark_tfrecord_amd.torch_data import (FixedLen, Padded, Padded2D,
                                               TFRecordBatchDataset,
                                               TFRecordIterableDataset)

    rank, world = _env_world()
    if not torch.cuda.is_available():
        raise SystemExit("collate needs the GPU engine")
    rows, B = args.rows, 8192
    d = _workdir("collate", rank)
    out = os.path.join(d, "t")
    stf.write_tfrecord(_flagship_table(rows, 9 + rank), out,
                       record_type="Example", num_shards=8, engine="gpu")
    schema = stf.read_tfrecord(out, engine="gpu").schema
    spec = {"id": FixedLen(), "ints": Padded(8), "floats": FixedLen(16),
            "tokens": Padded2D(2, 12)}
    part = args.collate_part

    # -- collation alone, one decoded shard --------------------------------
    shard = gpu_engine.read_file_to_batch(P.list_data_files(out)[0], schema,
                                          "Example", True)
    R = shard.num_rows
    ranges = [(lo, min(R, lo + B)) for lo in range(0, R, B)]
    co = Collator(schema, spec, "gpu")
    co.set_window([shard])
    sels = [(np.zeros(hi - lo, np.int32), np.arange(lo, hi, dtype=np.int64))
            for lo, hi in ranges]

    def run_kernel():
        for slot, row in sels:
            outs, status = co.run(slot, row)
        assert status[0] == (1 << 64) - 1
        return outs

    def run_torch():
        for lo, hi in ranges:
            outs = _torch_collate(shard, lo, hi, torch)
        assert not bool(outs["_bad"])  # the one wait, as the kernel's
        return outs

    alone = {"kernel": run_kernel, "torch": run_torch}
    if part in ("kernel", "torch", "none"):
        alone = {k: f for k, f in alone.items() if k == part}
    if part == "all":
        a, b = run_kernel(), run_torch()
        for k in a:  # the two collations agree
            assert torch.equal(a[k], b[k]), k
    el_alone = dict.fromkeys(alone, 0.0)
    for f in alone.values():
        f()  # warm-up
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, f in alone.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            el_alone[k] += time.perf_counter() - t0
    for k, t in el_alone.items():
        _emit(rank, f"rows/sec collate alone ({k}), one shard", R * args.reps / t,
              "rows/s", {"rows": R, "batch": B, "batches": len(ranges),
                         "reps": args.reps, "part": k,
                         "ms_per_batch": round(
                             t * 1e3 / (args.reps * len(ranges)), 4),
                         "engine": "gpu"}, t, 1)
    if part != "all":
        shutil.rmtree(d, ignore_errors=True)
        return

    # -- whole pipelines ---------------------------------------------------
    def ragged():
        n = 0
        for b in TFRecordIterableDataset(out, schema=schema, batch_rows=B,
                                         engine="gpu"):
            n += b["id"].numel()
        return n

    stats = {}

    def dense(window, prefetch=1):
        def run():
            ds = TFRecordBatchDataset(out, spec, batch_size=B,
                                      shuffle_window=window, engine="gpu",
                                      schema=schema, prefetch=prefetch)
            n = 0
            for b in ds:
                n += b["id"].shape[0]
            stats[window] = dict(ds.last_stats)
            return n
        return run

    # the slots of a window drain at about the same time, so (c) refills in
    # bursts of 4 decodes; the last mode lets the decode thread run 4 ahead
    # (measured: no gain, profiles/RESULTS.md "Batch collation")
    modes = {"a: TFRecordIterableDataset (ragged)": ragged,
             "b: TFRecordBatchDataset shuffle_window=0": dense(0),
             "c: TFRecordBatchDataset shuffle_window=4": dense(4),
             "c4: TFRecordBatchDataset shuffle_window=4 prefetch=4":
                 dense(4, 4)}
    el = dict.fromkeys(modes, 0.0)
    for f in modes.values():
        assert f() == rows  # warm-up
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for m, f in modes.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            el[m] += time.perf_counter() - t0
    ta = el["a: TFRecordIterableDataset (ragged)"]
    for m, t in el.items():
        w = None if m.startswith("a") else 0 if m.startswith("b") else 4
        _emit(rank, f"rows/sec training batches, {m}", rows * args.reps / t,
              "rows/s", {"rows": rows, "files": 8, "batch": B,
                         "over_ragged": round(ta / t, 3),
                         "last_stats": stats.get(w), "engine": "gpu",
                         "reps": args.reps}, t, 1)
    shutil.rmtree(d, ignore_errors=True)


BENCHES = {"plumbing": bench_plumbing, "partitionby": bench_partitionby,
           "infer": bench_infer, "gzip_bytearray": bench_gzip_bytearray,
           "gzip_write": bench_gzip_write,
           "gzip_foreign": bench_gzip_foreign,
           "snappy": bench_snappy, "snappy_write": bench_snappy_write,
           "collate": bench_collate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", choices=list(BENCHES) + ["all"])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--collate-part", default="all",
                    choices=["all", "kernel", "torch", "none"],
                    help="collate: run only one collation-alone loop "
                         "(for a kernel trace of its own)")
    args = ap.parse_args()
    names = list(BENCHES) if args.which == "all" else [args.which]
    for n in names:
        BENCHES[n](args)


if __name__ == "__main__":
    main()
