"""GPU engine: gfx950 kernel pipeline orchestration.

Decode: sliced H2D (file-mapping DMA); per arrived slice, under the later
slices' DMA and with one host round trip (a snapshot of the device state):
two-pass frame scan -> chain check -> fused structure-scan+CRC -> ranged
rocprim prefix sums -> gated extract_fields, which writes the device
wire-form columns whole (values, elem_off, sub_off, presence).
decode_device is the same pipeline over a whole resident image.
Encode: device wire-form -> size_records -> prefix sum -> record-range
sliced fused emit+CRC overlapped with the D2H DMA into the file mapping.

All kernels launch on the torch current stream, forming one in-order
pipeline; file DMA runs on two side streams gated by events (SURVEY.md §7
step 3). See docs/KERNELS.md for per-kernel design notes and measurements.
"""

from __future__ import annotations

import os
import threading
import warnings
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from .. import _native
from . import stream_plan
from ..columnar import RecordBatch, WireColumn, schema_blob, wire_fields
from ..schema import KIND_BYTES, KIND_FLOAT, KIND_INT64, StructType, is_sequence_field, wire_kind_of

FMT = {"Example": _native.FMT_EXAMPLE, "SequenceExample": _native.FMT_SEQUENCE}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(x, dtype, device="cuda") -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    arr = np.ascontiguousarray(x)
    # arrow buffers are read-only and torch warns on wrapping them; the
    # wrapped tensor is only ever read (the .to() below copies to device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return torch.as_tensor(arr, dtype=dtype).to(device)


def check_native():
    if not getattr(_native, "HAS_GPU_KERNELS", False):
        raise RuntimeError("_native was built without HIP kernels; rebuild "
                           "with build_native.py before using the GPU engine")


# ---------------------------------------------------------------------------
# Pinned staging buffers: host<->device copies through pageable memory run at
# ~8 GB/s on this platform vs ~57 GB/s pinned (measured, exp/exp_probe.py).
# One reusable pinned buffer per purpose, grown geometrically.
# ---------------------------------------------------------------------------

_pinned_tls = threading.local()


def pinned_buffer(tag: str, nbytes: int) -> torch.Tensor:
    """Reusable pinned staging buffer for `tag`, grown geometrically.

    Pools are THREAD-LOCAL: a tag names a pipeline slot (e.g. the writer's
    rotating D2H buffers), and two user threads writing concurrently must
    not stage through the same memory — one thread's host-side read of the
    view races the other's next async copy into it. Thread-local storage
    also frees a thread's buffers when it exits."""
    pool = getattr(_pinned_tls, "pool", None)
    if pool is None:
        pool = _pinned_tls.pool = {}
    buf = pool.get(tag)
    if buf is None or buf.numel() < nbytes:
        cap = max(nbytes, int((buf.numel() if buf is not None else 1 << 20) * 1.5))
        buf = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        pool[tag] = buf
    return buf


_CHUNK = 64 << 20  # 64 MiB: overlap file IO with PCIe copies chunkwise
# engine knobs: overridable via env for tuning
# 32 MiB: the work of the last slice(s) is the decode tail. With one host
# round trip per slice the kernel chain of a slice fits under its copy down
# to 16 MiB, but the step no longer moves with the slice size (measured
# 32/24/20/16 MiB: 8.50/8.48/8.54/8.52 ms per flagship step, spread 0.09), so
# the default stays.
_READ_SLICE = int(os.environ.get("TFREC_READ_SLICE", 32 << 20))
# Each slice is copied half on either DMA stream. The streams share the
# link, so whole slices alternating between them land in pairs and the tail
# holds a pair's work (9.18 ms); TFREC_READ_SPLIT=0 restores that.
_SPLIT_SLICES = os.environ.get("TFREC_READ_SPLIT", "1") != "0"
_WRITE_SLICES = int(os.environ.get("TFREC_WRITE_SLICES", 8))
# Streamed decode: the pipelined reader discovers, chain-checks and
# structure-scans each slice's records while later slices are still in DMA
# flight. TFREC_STREAM_DECODE=0 forces the unstreamed path (COUNT under the
# DMA, everything else after the last slice).
_STREAM_DECODE = os.environ.get("TFREC_STREAM_DECODE", "1") != "0"
# Row buffers of the streamed path are sized from the record density of the
# first slice that yields records, times this headroom; a launch that would
# not fit regrows them by copy.
_STREAM_HEADROOM = float(os.environ.get("TFREC_STREAM_HEADROOM", 1.125))
# Also run the value extraction per arrived slice (0: once over the whole
# file after the last slice).
_STREAM_EXTRACT = os.environ.get("TFREC_STREAM_EXTRACT", "1") != "0"
# msync mapped-DMA writes before the publishing rename (durability parity
# with write_file_atomic's fsync; near-free on tmpfs). TFREC_SYNC=0 disables.
_SYNC_WRITES = os.environ.get("TFREC_SYNC", "1") != "0"


def read_file_to_device(path: str, device="cuda") -> torch.Tensor:
    """File -> HBM. Fast path: hipHostRegister'd mmap of the file, one DMA
    straight out of the page cache (zero host memcpy). Fallback: pinned
    staging chunks through the native pread worker pool."""
    n = os.path.getsize(path)
    dev_t = torch.empty(max(n, 1), dtype=torch.uint8, device=device)[:n]
    if n:
        ptr, pinned = _native.file_mmap_pinned(path, n, False)
        if pinned:
            _multi_dma(dev_t.data_ptr(), ptr, n, _native.gpu_memcpy_h2d,
                       after_main=True)
            return dev_t
    return _read_file_staged(path, dev_t)


_copy_streams: Optional[list] = None


def _dma_streams() -> list:
    global _copy_streams
    if _copy_streams is None:
        _copy_streams = [torch.cuda.Stream() for _ in range(2)]
    return _copy_streams


def _multi_dma(dst: int, src: int, n: int, fn, after_main: bool):
    """Issue one big pinned<->HBM copy on up to TWO side streams: measured
    (exp/exp_dma.py) 56 GB/s each way at k<=2 — k=4 overcommits the SDMA
    engines and falls back to ~37 GB/s shader blits. Side streams keep the
    copy off the compute stream. after_main=True orders the copies after
    current-stream work and makes the main stream wait for completion;
    False blocks until the copies land."""
    streams = _dma_streams()
    main = torch.cuda.current_stream()
    k = min(len(streams), max(1, n // (16 << 20)))
    span = (n + k - 1) // k
    for i in range(k):
        o = i * span
        m = min(span, n - o)
        s = streams[i]
        s.wait_stream(main)
        fn(dst + o, src + o, m, s.cuda_stream)
    if after_main:
        for i in range(k):
            main.wait_stream(streams[i])
    else:
        for i in range(k):
            streams[i].synchronize()


def _read_file_staged(path: str, dev: torch.Tensor) -> torch.Tensor:
    n = dev.numel()
    buf = pinned_buffer("fread", min(n, 2 * _CHUNK) or 1)
    ev = [torch.cuda.Event(), torch.cuda.Event()]
    fd = os.open(path, os.O_RDONLY)
    try:
        pos = 0
        which = 0
        while pos < n:
            m = min(_CHUNK, n - pos)
            ev[which].synchronize()  # prior H2D from this half must be done
            _native.pread_parallel(fd, buf.data_ptr() + which * _CHUNK, m, pos)
            dev[pos:pos + m].copy_(buf[which * _CHUNK:which * _CHUNK + m],
                                   non_blocking=True)
            ev[which].record()
            pos += m
            which ^= 1 if n > _CHUNK else 0
    finally:
        os.close(fd)
    return dev


def _upload_files(dst: torch.Tensor, entries):
    """Whole files -> their slices of `dst`: entries = [(path, nbytes,
    dst_offset)], zero-length files skipped. Each file DMAs from the page
    cache (pinned mmap) on one of the side streams, or comes through the
    staged read where its mapping cannot be pinned; the main stream then
    waits for every side stream used. A side stream first waits for the
    main stream: `dst` is usually fresh from the caching allocator, which
    may hand back memory that an earlier main-stream kernel still reads.
    This is the one upload of every multi-file read. The raw branch of
    read_files_to_batch once had its own copy that left this wait out, so
    its copies could race such a kernel."""
    main = torch.cuda.current_stream()
    streams = _dma_streams()
    used = []
    for k, (path, nbytes, off) in enumerate(entries):
        if not nbytes:
            continue
        ptr, pinned = _native.file_mmap_pinned(path, nbytes, False)
        if pinned:
            st = streams[k % len(streams)]
            st.wait_stream(main)
            _native.gpu_memcpy_h2d(dst.data_ptr() + off, ptr, nbytes,
                                   st.cuda_stream)
            used.append(st)
        else:
            _read_file_staged(path, dst[off:off + nbytes])
    for st in set(used):
        main.wait_stream(st)


def _upload_group(items, device):
    """The files of a group's items [(path, ...)] back to back in one fresh
    device buffer: (buffer, each file's offset in it, each file's size)."""
    sizes = [os.path.getsize(it[0]) for it in items]
    offs = [0]
    for n in sizes[:-1]:
        offs.append(offs[-1] + n)
    total = sum(sizes)
    comp = torch.empty(max(total, 1), dtype=torch.uint8, device=device)[:total]
    _upload_files(comp, [(it[0], n, o) for it, n, o in zip(items, sizes, offs)])
    return comp, offs, sizes


def device_to_file(img: torch.Tensor, path: str):
    """HBM file image -> file. Fast path: the file is sized, mmap'd and
    hipHostRegister'd, then ONE D2H DMA writes HBM straight into the file's
    page-cache pages (tmpfs: that IS the storage; disk FS: the kernel
    writes back). Fallback: pinned staging + parallel pwrite (a plain
    multi-threaded pwrite to one file serializes on the inode mutex)."""
    n = img.numel()
    if n == 0:
        open(path, "wb").close()
        return
    # Always map+register: on a FRESH file every write strategy is
    # page-allocation-bound anyway (~6-7 GB/s measured across register+DMA,
    # pwrite pool, mmap memcpy and plain write — exp/exp_freshwrite.py),
    # and the registered mapping makes every REWRITE a pure ~56 GB/s DMA.
    ptr, pinned = _native.file_mmap_pinned(path, n, True)
    if pinned:
        _multi_dma(ptr, img.data_ptr(), n, _native.gpu_memcpy_d2h,
                   after_main=False)
        if _SYNC_WRITES:
            _native.file_mmap_sync(path)
        return
    _write_file_staged(img, path)


def _write_file_staged(img: torch.Tensor, path: str):
    """Fallback writer when hipHostRegister is unavailable: D2H chunks into
    pinned staging overlapped with plain write()s (single-threaded write
    beats a pwrite pool on the per-inode mutex)."""
    n = img.numel()
    buf = pinned_buffer("fwrite", min(n, 2 * _CHUNK) or 1)
    ev = [torch.cuda.Event(), torch.cuda.Event()]
    fd = os.open(path, os.O_RDWR | os.O_CREAT, 0o644)
    try:
        pos = 0
        which = 0
        # prefetch chunk 0
        m0 = min(_CHUNK, n)
        if n:
            buf[0:m0].copy_(img[0:m0], non_blocking=True)
            ev[0].record()
        while pos < n:
            m = min(_CHUNK, n - pos)
            nxt = pos + m
            nwhich = which ^ (1 if n > _CHUNK else 0)
            if nxt < n:  # start next D2H before blocking on this chunk
                m2 = min(_CHUNK, n - nxt)
                buf[nwhich * _CHUNK:nwhich * _CHUNK + m2].copy_(
                    img[nxt:nxt + m2], non_blocking=True)
                ev[nwhich].record()
            ev[which].synchronize()
            _native.pwrite_parallel(fd, buf.data_ptr() + which * _CHUNK, m, pos)
            pos = nxt
            which = nwhich
        os.ftruncate(fd, n)
        if _SYNC_WRITES:
            os.fsync(fd)
    finally:
        os.close(fd)


# ---------------------------------------------------------------------------
# Prefix sums: rocprim decoupled-lookback scans (native). torch.cumsum's
# innermost-dim kernel launches one block per row — 2.5 ms on a [4, 1M] int64
# scan (profiles/r01_kernel_stats.txt) vs memory-speed here.
# ---------------------------------------------------------------------------

_scan_ws = {}


def _scan_workspace(n: int, device) -> torch.Tensor:
    key = (device.index if hasattr(device, "index") else 0)
    need = _native.gpu_scan_temp_bytes(max(n, 1))
    ws = _scan_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(int(need * 2), dtype=torch.uint8, device=device)
        _scan_ws[key] = ws
    return ws


def _excl_sum_into(out_ptr: int, in_ptr: int, stride: int, n: int, device):
    ws = _scan_workspace(n, device)
    _native.gpu_excl_sum_strided(ws.data_ptr(), ws.numel(), in_ptr, stride,
                                 out_ptr, n, _stream())


def _stat_scan_workspace(R: int, F: int, device) -> torch.Tensor:
    key = ("stat", device.index if hasattr(device, "index") else 0)
    need = _native.gpu_stat_scan_temp_bytes(R, F)
    ws = _scan_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(int(need * 2) or 1, dtype=torch.uint8, device=device)
        _scan_ws[key] = ws
    return ws


def excl_sum(t: torch.Tensor) -> torch.Tensor:
    """Contiguous 1-D int64 tensor -> (n+1)-long exclusive scan, total at [-1]."""
    n = t.numel()
    out = torch.empty(n + 1, dtype=torch.int64, device=t.device)
    _excl_sum_into(out.data_ptr(), t.data_ptr(), 1, n, t.device)
    return out


def device_to_bytes(img: torch.Tensor) -> bytes:
    n = img.numel()
    buf = pinned_buffer("d2h", n)
    buf[:n].copy_(img, non_blocking=True)
    torch.cuda.synchronize()
    return buf.numpy()[:n].tobytes()


def device_to_pinned_view(img: torch.Tensor, tag: str = "d2h_img") -> np.ndarray:
    """One link-speed D2H of a device image into the reusable pinned buffer;
    returns a numpy VIEW of it (valid until the tag's next use). Partitioned
    writes slice this view per partition file — registering a fresh mmap per
    part file costs ~0.16 ms/MB in hipHostRegister alone, ~10x the bytes'
    DMA time for many small fresh files (r01 config-3 cliff)."""
    n = img.numel()
    buf = pinned_buffer(tag, n)
    buf[:n].copy_(img, non_blocking=True)
    torch.cuda.synchronize()
    return buf.numpy()[:n]


# ---------------------------------------------------------------------------
# GPU frame scan: parallel frame-boundary discovery + chain validation.
# ---------------------------------------------------------------------------

def scan_frames_device(data: torch.Tensor):
    """Device file image -> (payload_off, payload_len) device tensors.

    Every byte position is CRC-tested as a candidate frame head in parallel
    (two-pass count/emit — candidates come out position-sorted by
    construction, no device sort); the chain pos[k+1] == pos[k]+16+len[k]
    must hold exactly — a false positive (p=2^-32/byte) or a torn file
    breaks it and raises."""
    check_native()
    N = data.numel()
    device = data.device
    if N == 0:
        z = torch.zeros(0, dtype=torch.int64, device=device)
        return z, z.clone()
    B = _native.gpu_frame_scan_blocks(0, N)
    block_counts = torch.empty(B, dtype=torch.int64, device=device)
    _native.gpu_frame_scan_count(data.data_ptr(), N, 0, N, 0,
                                 block_counts.data_ptr(), _stream())
    off, lens, _ = _emit_and_chain(data, [(0, N)], block_counts, N)
    return off, lens


def _emit_and_chain(data, ranges, block_counts, N):
    """Prefix-sum the per-block candidate counts, emit the (sorted)
    candidates at exact offsets, then validate the frame chain. Returns
    (payload_off, payload_len, clean) — clean=False when a false-positive
    candidate had to be stitched out on host."""
    device = data.device
    block_off = excl_sum(block_counts)
    C = int(block_off[-1].item())
    if C == 0:
        raise RuntimeError("corrupt TFRecord: no valid frame header found")
    pos = torch.empty(C, dtype=torch.int64, device=device)
    lens = torch.empty(C, dtype=torch.int64, device=device)
    base = 0
    for s, e in ranges:
        _native.gpu_frame_scan_emit(data.data_ptr(), N, s, e, base,
                                    block_off.data_ptr(), pos.data_ptr(),
                                    lens.data_ptr(), _stream())
        base += _native.gpu_frame_scan_blocks(s, e)
    # chain check fused to ONE device scalar -> one sync
    expect_next = pos + 16 + lens
    ok = bool(((pos[0] == 0) & (expect_next[-1] == N)
               & (expect_next[:-1] == pos[1:]).all()).item())
    if not ok:
        # rare: false-positive candidate inside a payload — stitch on host
        pos_h = pos.cpu().numpy()
        len_h = lens.cpu().numpy()
        keep = []
        cur = 0
        pmap = {int(p): i for i, p in enumerate(pos_h)}
        while cur < N:
            i = pmap.get(cur)
            if i is None:
                raise RuntimeError(
                    f"corrupt TFRecord: broken frame chain at offset {cur}")
            keep.append(i)
            cur = int(pos_h[i] + 16 + len_h[i])
        sel = torch.as_tensor(np.asarray(keep, np.int64), device=device)
        pos = pos[sel]
        lens = lens[sel]
    return pos + 12, lens, ok


# ---------------------------------------------------------------------------
# Decode
# ---------------------------------------------------------------------------

def crc_verify_device(data: torch.Tensor, off: torch.Tensor, lens: torch.Tensor,
                      avg_bytes: int = 0):
    """Raise on any bad frame CRC (parallel over records; records larger
    than ~8 KB verify one-per-wavefront with GF(2)-combined chunk CRCs)."""
    R = off.numel()
    if R == 0:
        return
    if not avg_bytes:
        avg_bytes = max(0, (data.numel() // R) - 16)
    err = torch.full((1,), -1, dtype=torch.int64, device=data.device)  # all-ones
    _native.gpu_crc_verify(data.data_ptr(), off.data_ptr(), lens.data_ptr(), R,
                           err.data_ptr(), _stream(), avg_bytes)
    bad = int(err.item())  # syncs
    if bad != -1:
        raise RuntimeError(
            f"corrupt TFRecord: bad CRC in record {bad - 1 if bad > 0 else bad}")


def decode_device(data: torch.Tensor, off: torch.Tensor, lens: torch.Tensor,
                  schema: StructType, record_type: str,
                  verify_crc: bool = True) -> RecordBatch:
    """Decode framed records already resident in HBM into device wire-form."""
    check_native()
    device = data.device
    R = off.numel()
    fields = wire_fields(schema)
    F = len(fields)
    if verify_crc and record_type == "ByteArray":
        crc_verify_device(data, off, lens)

    if record_type == "ByteArray":
        dst_off = excl_sum(lens.contiguous())
        total = int(dst_off[-1].item())
        out = torch.empty(total, dtype=torch.uint8, device=device)
        if R:
            _native.gpu_gather_payloads(data.data_ptr(), off.data_ptr(),
                                        lens.data_ptr(), dst_off.data_ptr(), R,
                                        out.data_ptr(), _stream(), total // R)
        col = WireColumn(kind=KIND_BYTES, is_seq=False,
                         presence=torch.ones(R, dtype=torch.uint8, device=device),
                         row_off=torch.arange(R + 1, dtype=torch.int64, device=device),
                         values=out, elem_off=dst_off)
        return RecordBatch(schema, [col], R)

    if F == 0 or R == 0:
        cols = [WireColumn(wire_kind_of(f.dataType), is_sequence_field(f.dataType),
                           torch.zeros(R, dtype=torch.uint8, device=device),
                           torch.zeros(R + 1, dtype=torch.int64, device=device),
                           torch.zeros(0, dtype=torch.int64, device=device))
                for f in fields]
        return RecordBatch(schema, cols, R)

    blob = _schema_blob_device(schema, device)
    # FieldStat[R][F] as int64 [R,F,6]: pos,len,nvals,nbytes,nlists,(kind|err)
    stats = torch.empty((R, F, 6), dtype=torch.int64, device=device)
    # err buffers are int32[2]: (codec error code, 1 + offending record index)
    err = torch.zeros(2, dtype=torch.int32, device=device)
    # frame CRC verification is FUSED into the structure scan: the record
    # bytes are CRC'd while L2-hot from the parse. (A concurrent side-stream
    # CRC pass was tried and reverted: it is a second full read of the
    # file, and the fused form has ~1 ms less total GPU work per 215 MB.)
    # NOTE: for Example/SequenceExample the CRC stays FUSED into the scan at
    # any record size — the serial protobuf parse dominates huge records, so
    # a separate wave-CRC pass only adds a second full read (measured).
    # The wave CRC/copy kernels serve the parse-free ByteArray paths.
    crc_err = None
    fuse_crc = verify_crc
    if fuse_crc:
        crc_err = torch.full((1,), -1, dtype=torch.int64, device=device)
    # average record size steers the one-per-lane vs one-per-wave kernels
    avg_bytes = max(0, (data.numel() // R) - 16) if R else 0
    _native.gpu_scan_records(data.data_ptr(), off.data_ptr(), lens.data_ptr(),
                             R, FMT[record_type], blob.data_ptr(), F,
                             stats.data_ptr(), err.data_ptr(),
                             crc_err.data_ptr() if fuse_crc else 0,
                             _stream(), avg_bytes)

    # Per-field exclusive prefix sums ([F, R+1] x 3 planes) in ONE rocprim
    # launch: a head-flag segmented scan over the [F*R] triple sequence
    # scatters into all planes (3F separate scans cost 6F launches).
    val_base = torch.empty((F, R + 1), dtype=torch.int64, device=device)
    byte_base = torch.empty((F, R + 1), dtype=torch.int64, device=device)
    list_base = torch.empty((F, R + 1), dtype=torch.int64, device=device)
    val_base[:, 0] = 0
    byte_base[:, 0] = 0
    list_base[:, 0] = 0
    ws = _stat_scan_workspace(R, F, device)
    _native.gpu_stat_scans(ws.data_ptr(), ws.numel(), stats.data_ptr(), R, F,
                           val_base.data_ptr(), byte_base.data_ptr(),
                           list_base.data_ptr(), _stream())
    totals = torch.stack([val_base[:, -1], byte_base[:, -1], list_base[:, -1]])
    totals_h = totals.cpu()  # one sync for all allocations
    _raise_scan_errors(int(crc_err.item()) if fuse_crc else -1,
                       int(err[0].item()), int(err[1].item()))
    # every total is known: bytes_seen == total_bytes sizes the buffers exactly
    vals = _FieldValues(fields, data.numel(), device)
    vals.reserve(totals_h, data.numel())
    presence = torch.empty((F, R), dtype=torch.uint8, device=device)
    vals.extract(data, stats, (val_base, byte_base, list_base), presence, 0, R,
                 _MetaTable(F, device), err, avg_bytes)
    vals.confirm(totals_h)
    cols = vals.columns(presence, val_base, list_base, R)
    if int(err[0].item()) != 0:
        _raise_extract_error(int(err[0].item()), int(err[1].item()))
    return RecordBatch(schema, cols, R)


_schema_blobs = {}


def _schema_blob_device(schema: StructType, device) -> torch.Tensor:
    """Device copy of the schema blob, cached per (blob bytes, device): a
    schema does not change between reads, and the upload is a pageable,
    synchronous copy."""
    raw = bytes(schema_blob(schema))
    key = (raw, str(torch.device(device)))
    blob = _schema_blobs.get(key)
    if blob is None:
        if len(_schema_blobs) >= 64:
            _schema_blobs.clear()
        blob = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        _schema_blobs[key] = blob
    return blob


def _raise_scan_errors(crc_bad: int, rc: int, rec1: int):
    """Structure-scan outcome -> exception. crc_bad is the fused CRC word (-1
    clean, else 1 + first bad record), (rc, rec1) the codec error pair (rec1
    = 1 + offending record). A bad CRC takes precedence."""
    if crc_bad != -1:
        raise RuntimeError(f"corrupt TFRecord: bad CRC in record {crc_bad - 1}")
    if rc != 0:
        rec = rec1 - 1
        where = f" in record {rec}" if rec >= 0 else ""
        raise RuntimeError(f"TFRecord decode failed{where} (native error "
                           f"{rc}; kind mismatch or malformed record)")


def _raise_extract_error(rc: int, rec1: int):
    rec = rec1 - 1
    where = f" (record {rec})" if rec >= 0 else ""
    raise RuntimeError(f"TFRecord decode failed in value extraction"
                       f"{where} (native error {rc})")


class _MetaTable:
    """Device copy of gpu_extract_fields' field table, uploaded only when it
    differs from what the device copy last received: the pointers in it only
    change when a buffer regrows."""

    def __init__(self, F: int, device):
        self.dev = torch.empty(F * _native.gpu_devmeta_bytes(),
                               dtype=torch.uint8, device=device)
        self.last = None

    def changed(self, metas) -> bool:
        key = [tuple(m.items()) for m in metas]
        if key == self.last:
            return False
        self.last = key
        return True


class _FieldValues:
    """Per-field output buffers of the value extraction: values (int64 or
    float32), payload bytes and the finished elem_off / sub_off columns. The
    one place that builds the metas for gpu_extract_fields and turns filled
    buffers into WireColumns. reserve() grows every buffer to running totals
    the host has read: from the value density seen so far times
    _STREAM_HEADROOM (a regrow copies the filled prefix), which is exactly
    the totals once bytes_seen == total_bytes, as in decode_device."""

    # buffer -> (dtype, the totals row (values, bytes, lists) that sizes it,
    # slots past that total (the offset columns end with a sentinel), the
    # (kind, is_seq) of the fields that fill it)
    _BUFS = {"i64_vals": (torch.int64, 0, 0, lambda k, seq: k == KIND_INT64),
             "f32_vals": (torch.float32, 0, 0, lambda k, seq: k == KIND_FLOAT),
             "elem_off": (torch.int64, 0, 1, lambda k, seq: k == KIND_BYTES),
             "bytes_data": (torch.uint8, 1, 0, lambda k, seq: k == KIND_BYTES),
             "sub_off": (torch.int64, 2, 1, lambda k, seq: seq)}

    def __init__(self, fields, total_bytes: int, device):
        self.total_bytes = total_bytes
        self.device = device
        self.kinds = [wire_kind_of(f.dataType) for f in fields]
        self.seqs = [is_sequence_field(f.dataType) for f in fields]
        # running totals [3][F] of the rows whose extraction is confirmed
        self.filled = [[0] * len(fields) for _ in range(3)]
        self.bufs = [{k: torch.empty(0, dtype=d, device=device)
                      for k, (d, _, _, _) in self._BUFS.items()} for _ in fields]

    def reserve(self, totals, bytes_seen: int):
        """Room for the running totals ([3][F], host) seen bytes_seen bytes
        into the file."""
        for i, bufs in enumerate(self.bufs):
            for name, (_, dim, extra, fills) in self._BUFS.items():
                if not fills(self.kinds[i], self.seqs[i]):
                    continue
                need = int(totals[dim][i]) + extra
                old = bufs[name]
                cap = stream_plan.grown_capacity(
                    old.numel(), need, bytes_seen, self.total_bytes,
                    _STREAM_HEADROOM, min_unit=1)
                if cap == old.numel():
                    continue
                new = torch.empty(cap, dtype=old.dtype, device=self.device)
                k = min(self.filled[dim][i] + extra, old.numel())
                if k:
                    new[:k].copy_(old[:k])
                if old.numel():
                    last_read["regrows"] = last_read.get("regrows", 0) + 1
                bufs[name] = new

    def confirm(self, totals):
        """Every row up to the running totals `totals` has been extracted."""
        self.filled = [[int(totals[d][i]) for i in range(len(self.bufs))]
                       for d in range(3)]

    def extract(self, data, stats, planes, presence, r0: int, r1: int,
                meta: _MetaTable, err, avg_bytes: int, gate=None):
        """Launch the extraction of records [r0, r1) into the buffers as
        they are. stats is the FieldStat tensor from row 0, planes the three
        [F][stride] prefix-sum planes, presence the u8 [F][stride] plane.
        gate = (broken, crc, scan error, verdict) word addresses: the launch
        then checks on the device that the scan was clean and that the
        totals after row r1 fit, and writes nothing otherwise."""
        v, b, l = planes
        metas = []
        for i, bufs in enumerate(self.bufs):
            vals = bufs["i64_vals" if self.kinds[i] == KIND_INT64 else "f32_vals"]
            metas.append({
                "kind": self.kinds[i], "is_seq": 1 if self.seqs[i] else 0,
                **{name: t.data_ptr() for name, t in bufs.items()},
                "presence": presence[i].data_ptr(),
                "val_base": v[i].data_ptr(),
                "byte_base": b[i].data_ptr(),
                "list_base": l[i].data_ptr() if self.seqs[i] else 0,
                "cap_vals": vals.numel(),
                "cap_bytes": bufs["bytes_data"].numel(),
                "cap_elem_off": bufs["elem_off"].numel(),
                "cap_sub_off": bufs["sub_off"].numel(),
            })
        g_broken, g_crc, g_err, g_out = gate or (0, 0, 0, 0)
        _native.gpu_extract_fields(data.data_ptr(), r1 - r0, len(self.bufs),
                                   stats.data_ptr(), metas,
                                   meta.dev.data_ptr(), err.data_ptr(),
                                   _stream(), avg_bytes, r0=r0,
                                   upload=meta.changed(metas),
                                   gate_broken=g_broken, gate_crc=g_crc,
                                   gate_err=g_err, gate_out=g_out)

    def columns(self, presence, val_base, list_base, R: int) -> List[WireColumn]:
        """Wire columns of rows [0, R), all extracted and confirmed: views
        of what the kernels wrote, no launch. Row f of a plane cut to
        [:R + 1] is field f's row_off / list_off."""
        cols = []
        for i, bufs in enumerate(self.bufs):
            kind, seq = self.kinds[i], self.seqs[i]
            nv, nb, nl = (self.filled[d][i] for d in range(3))
            values = (bufs["i64_vals"][:nv] if kind == KIND_INT64 else
                      bufs["f32_vals"][:nv] if kind == KIND_FLOAT else
                      bufs["bytes_data"][:nb])
            cols.append(WireColumn(
                kind, seq, presence[i][:R], val_base[i][:R + 1], values,
                bufs["elem_off"][:nv + 1] if kind == KIND_BYTES else None,
                list_base[i][:R + 1] if seq else None,
                bufs["sub_off"][:nl + 1] if seq else None))
        return cols


def decode_buffer_device(data_np: np.ndarray, schema: StructType, record_type: str,
                         verify_crc: bool = True, device="cuda") -> RecordBatch:
    """Host bytes -> device batch (frame discovery AND decode on the GPU)."""
    data_np = np.ascontiguousarray(data_np, np.uint8)
    n = data_np.size
    stage = pinned_buffer("h2d", n)
    stage.numpy()[:n] = data_np
    data = torch.empty(n, dtype=torch.uint8, device=device)
    data.copy_(stage[:n], non_blocking=True)
    off, lens = scan_frames_device(data)
    return decode_device(data, off, lens, schema, record_type, verify_crc)


def read_file_to_batch(path: str, schema: StructType, record_type: str,
                       verify_crc: bool = True, device="cuda") -> RecordBatch:
    """Uncompressed file -> device batch (H2D sliced + overlapped with the
    frame scan; see read_file_to_batch_pipelined)."""
    return read_file_to_batch_pipelined(path, schema, record_type, verify_crc,
                                        device)


# ---------------------------------------------------------------------------
# Encode
# ---------------------------------------------------------------------------

def _col_ptrs(col: WireColumn) -> dict:
    def p(t):
        return t.data_ptr() if isinstance(t, torch.Tensor) and t.numel() else 0

    return {
        "kind": col.kind, "is_seq": 1 if col.is_seq else 0,
        "presence": p(col.presence), "row_off": p(col.row_off),
        "list_off": p(col.list_off) if col.list_off is not None else 0,
        "sub_off": p(col.sub_off) if col.sub_off is not None else 0,
        "elem_off": p(col.elem_off) if col.elem_off is not None else 0,
        "values_bytes": p(col.values) if col.kind == KIND_BYTES else 0,
        "values_i64": p(col.values) if col.kind == KIND_INT64 else 0,
        "values_f32": p(col.values) if col.kind == KIND_FLOAT else 0,
    }


def _check_emit_err(err: torch.Tensor):
    if int(err[0].item()) != 0:
        rec = int(err[1].item()) - 1
        where = f" in record {rec}" if rec >= 0 else ""
        raise RuntimeError(f"TFRecord encode failed: size/emit mismatch{where}")


def _size_records(batch: RecordBatch, record_type: str, device):
    """Upload the column table and size every record's frame. Returns
    (cols_dev, blob, psize, frame_off): the device column table, the schema
    blob, the per-record frame sizes and their (R+1)-long exclusive scan."""
    blob = _schema_blob_device(batch.schema, device)
    col_dicts = [_col_ptrs(c) for c in batch.columns]
    cols_dev = torch.empty(_native.gpu_devcols_bytes(len(col_dicts)),
                           dtype=torch.uint8, device=device)
    psize = torch.empty(batch.num_rows, dtype=torch.int64, device=device)
    _native.gpu_size_records(col_dicts, cols_dev.data_ptr(), blob.data_ptr(),
                             FMT[record_type], batch.num_rows,
                             psize.data_ptr(), _stream())
    return cols_dev, blob, psize, excl_sum(psize)


def encode_device(batch: RecordBatch, record_type: str) -> torch.Tensor:
    """Device wire-form batch -> framed file image as a device u8 tensor."""
    check_native()
    R = batch.num_rows
    device = batch.columns[0].presence.device if batch.columns else torch.device("cuda")
    if record_type == "ByteArray":
        col = batch.columns[0]
        lens = col.elem_off[1:] - col.elem_off[:-1]
        frame_off = excl_sum((lens + 16).contiguous())
        total = int(frame_off[-1].item())
        file = torch.empty(total, dtype=torch.uint8, device=device)
        if R:
            _native.gpu_frame_bytes(col.values.data_ptr(), col.elem_off.data_ptr(),
                                    frame_off.data_ptr(), R, file.data_ptr(),
                                    _stream(), (total // R) - 16)
        return file

    cols_dev, blob, _, frame_off = _size_records(batch, record_type, device)
    total = int(frame_off[-1].item())
    file = torch.empty(total, dtype=torch.uint8, device=device)
    err = torch.zeros(2, dtype=torch.int32, device=device)
    _native.gpu_emit_records(cols_dev.data_ptr(), blob.data_ptr(),
                             FMT[record_type], 0, R, frame_off.data_ptr(),
                             file.data_ptr(), err.data_ptr(), _stream(),
                             total // max(R, 1))
    _check_emit_err(err)
    return file


def write_batch_to_file(batch: RecordBatch, path: str,
                        record_type: str = "Example",
                        slices: Optional[int] = None) -> int:
    """Device batch -> framed TFRecord file, with the emit kernel sliced over
    record ranges so the D2H DMA of slice k streams to the file's mapped
    pages while slice k+1 is still being emitted (SURVEY.md §7 step 3:
    double-buffered transport overlapped with encode). Returns file bytes."""
    check_native()
    R = batch.num_rows
    if record_type == "ByteArray" or R == 0:
        img = encode_device(batch, record_type)
        device_to_file(img, path)
        return img.numel()
    device = batch.columns[0].presence.device
    cols_dev, blob, _, frame_off = _size_records(batch, record_type, device)
    S = max(1, min(slices if slices is not None else _WRITE_SLICES, R))
    ridx = [R * s // S for s in range(S + 1)]
    bounds = frame_off[ridx].cpu()  # one sync: slice byte bounds + total
    total = int(bounds[-1])
    file = torch.empty(total, dtype=torch.uint8, device=device)
    err = torch.zeros(2, dtype=torch.int32, device=device)
    ptr, pinned = _native.file_mmap_pinned(path, total, True)
    if not pinned:
        _native.gpu_emit_records(cols_dev.data_ptr(), blob.data_ptr(),
                                 FMT[record_type], 0, R, frame_off.data_ptr(),
                                 file.data_ptr(), err.data_ptr(), _stream(),
                                 total // R)
        _check_emit_err(err)
        _write_file_staged(file, path)
        return total
    main = torch.cuda.current_stream()
    streams = _dma_streams()
    for s in range(S):
        _native.gpu_emit_records(cols_dev.data_ptr(), blob.data_ptr(),
                                 FMT[record_type], ridx[s], ridx[s + 1],
                                 frame_off.data_ptr(), file.data_ptr(),
                                 err.data_ptr(), _stream(), total // R)
        b0, b1 = int(bounds[s]), int(bounds[s + 1])
        if b1 > b0:
            w = streams[s % len(streams)]
            w.wait_stream(main)
            _native.gpu_memcpy_d2h(ptr + b0, file.data_ptr() + b0, b1 - b0,
                                   w.cuda_stream)
    for w in streams:
        w.synchronize()
    if _SYNC_WRITES:
        _native.file_mmap_sync(path)
    _check_emit_err(err)
    return total


# what the last read_file_to_batch_pipelined call on a registered mapping did:
# path = "streamed" | "fallback" (streamed attempt abandoned) | "unstreamed"
# (TFREC_STREAM_DECODE=0), the slice count, the buffer regrows and how often
# the streamed path blocked on the device (host_waits)
last_read = {}

# words of the streamed read's status block
_ST_BROKEN, _ST_CRC, _ST_ERR, _ST_XERR, _ST_NOEXT, _ST_CARRY = 0, 1, 2, 3, 4, 5


class _StreamStatus:
    """One int64 status block per streamed read: the broken-chain flag, the
    fused CRC word (all-ones = clean), the scan's int32 codec error pair, the
    extraction's, the extraction gate's verdict (1 = the last gated launch
    wrote nothing), then one word per chain launch: word k is the end of the
    k-th launch's last candidate and the carry into the next (the carry into
    the first is 0)."""

    def __init__(self, max_chains: int, device):
        self.words = torch.zeros(_ST_CARRY + 1 + max_chains, dtype=torch.int64,
                                 device=device)
        self.words[_ST_CRC] = -1
        self.err = self.words[_ST_ERR:_ST_ERR + 1].view(torch.int32)
        self.xerr = self.words[_ST_XERR:_ST_XERR + 1].view(torch.int32)

    def addr(self, word: int) -> int:
        return self.words.data_ptr() + word * 8

    def carry_addr(self, k: int) -> int:
        """Carry into chain launch k == end of launch k - 1."""
        return self.addr(_ST_CARRY + k)


class _Snapshot:
    """Host copy of one gpu_stream_snapshot block: the slice's candidate
    count, the status head words, the chain end so far and the running
    totals [3][F] at the row the snapshot was taken for."""

    def __init__(self, h: np.ndarray, F: int):
        self.count = int(h[0])
        st = h[1:1 + _ST_CARRY]
        self.broken = int(st[_ST_BROKEN]) != 0
        pair = st[_ST_ERR:_ST_ERR + 1].view(np.int32)
        # (crc word, codec rc, 1 + offending record) of the rows scanned
        self.scan_error = (int(st[_ST_CRC]), int(pair[0]), int(pair[1]))
        xpair = st[_ST_XERR:_ST_XERR + 1].view(np.int32)
        self.xerr = (int(xpair[0]), int(xpair[1]))
        self.refused = int(st[_ST_NOEXT]) != 0
        self.chain_end = int(h[1 + _ST_CARRY])
        self.totals = h[2 + _ST_CARRY:].reshape(3, F) if F else None


class _StreamRows:
    """Row-indexed buffers of one streamed read: candidate pos/len, payload
    off and (F > 0) the FieldStat rows, the prefix-sum planes and the
    presence plane. Sized from the record density of the first slice that
    yields candidates times _STREAM_HEADROOM; reserve() is called on the
    host before every launch that writes rows, and regrows by copying the
    filled rows when the launch would not fit."""

    def __init__(self, total_bytes: int, F: int, device):
        self.total_bytes = total_bytes
        self.F = F
        self.device = device
        self.cap = 0
        self.pos = self.lens = self.off = self.stats = None
        # exclusive prefix sums of nvals/nbytes/nlists, [F][cap + 1] each;
        # row f cut to [:R + 1] is the contiguous row_off of field f
        self.planes = None
        # u8 [F][cap], written by the extraction
        self.presence = None

    def _alloc(self, cap: int):
        i64 = dict(dtype=torch.int64, device=self.device)
        planes = presence = None
        if self.F:
            planes = [torch.empty((self.F, cap + 1), **i64) for _ in range(3)]
            for t in planes:
                t[:, 0] = 0
            presence = torch.empty((self.F, cap), dtype=torch.uint8,
                                   device=self.device)
        return (torch.empty(cap, **i64), torch.empty(cap, **i64),
                torch.empty(cap, **i64),
                torch.empty((cap, self.F, 6), **i64) if self.F else None,
                planes, presence)

    def cand_ptrs(self, c: int):
        """Addresses of candidate c's (pos, len, off) entries."""
        return (self.pos.data_ptr() + c * 8, self.lens.data_ptr() + c * 8,
                self.off.data_ptr() + c * 8)

    def row_ptrs(self, r: int):
        """Addresses of record r's (off, len, FieldStat row) entries."""
        return (self.off.data_ptr() + r * 8, self.lens.data_ptr() + r * 8,
                self.stats.data_ptr() + r * self.F * 48)

    def scan_stats(self, r0: int, r1: int):
        """Ranged stat prefix sums over scanned rows [r0, r1): carries on
        from the running totals at plane[f][r0]."""
        ws = _stat_scan_workspace(r1 - r0, self.F, self.device)
        v, b, l = self.planes
        _native.gpu_stat_scans(ws.data_ptr(), ws.numel(),
                               self.stats.data_ptr(), r1, self.F, v.data_ptr(),
                               b.data_ptr(), l.data_ptr(), _stream(), r0=r0,
                               r1=r1, stride=self.cap + 1)

    def reserve(self, need: int, n_cand: int, n_scanned: int, bytes_seen: int):
        """Make room for `need` rows; rows [0, n_cand) of pos/len/off and
        [0, n_scanned) of stats, planes and presence are live."""
        cap = stream_plan.grown_capacity(self.cap, need, bytes_seen,
                                         self.total_bytes, _STREAM_HEADROOM)
        if cap == self.cap:
            return
        pos, lens, off, stats, planes, presence = self._alloc(cap)
        if n_cand:
            pos[:n_cand].copy_(self.pos[:n_cand])
            lens[:n_cand].copy_(self.lens[:n_cand])
            off[:n_cand].copy_(self.off[:n_cand])
        if n_scanned and stats is not None:
            stats[:n_scanned].copy_(self.stats[:n_scanned])
            for new, old in zip(planes, self.planes):
                new[:, :n_scanned + 1].copy_(old[:, :n_scanned + 1])
            presence[:, :n_scanned].copy_(self.presence[:, :n_scanned])
        self.pos, self.lens, self.off, self.stats = pos, lens, off, stats
        self.planes, self.presence = planes, presence
        if self.cap:
            last_read["regrows"] = last_read.get("regrows", 0) + 1
        self.cap = cap


class _StreamedRead:
    """State and steps of one streamed read over `data`, whose slices are
    still landing. step() runs once per landed slice and blocks on the device
    once: a snapshot that brings the slice's candidate count together with
    what became of the previous slice's launches. Everything it then
    launches (EMIT, chain, structure scan, stat scan, extraction) decides on
    the device whether it may run: the scan looks at the broken-chain word,
    the extraction at extract_gate_kernel's verdict. finish() runs after the
    last slice."""

    def __init__(self, data: torch.Tensor, nslices: int, schema: StructType,
                 record_type: str, verify_crc: bool):
        device = data.device
        self.data = data
        self.n = data.numel()
        self.schema = schema
        self.record_type = record_type
        self.verify_crc = verify_crc
        fields = wire_fields(schema)
        F = self.F = len(fields)
        # ByteArray and field-less schemas only stream the frame discovery
        self.do_scan = record_type != "ByteArray" and F > 0
        self.status = _StreamStatus(nslices, device)
        self.rows = _StreamRows(self.n, F if self.do_scan else 0, device)
        if self.do_scan:
            self.blob = _schema_blob_device(schema, device)
            self.vals = _FieldValues(fields, self.n, device)
            self.meta = _MetaTable(F, device)
        self.C = 0       # chained candidates so far
        self.nchain = 0  # chain launches so far
        self.r_done = 0  # records whose structure scan has been launched
        self.x_done = 0  # records whose extraction is confirmed
        self.x_pending = None  # end row of a gated extraction not yet confirmed
        self.sized = False  # value buffers sized from a measured density
        self.bytes_done = 0  # bytes the scanned rows lie in
        self.clean = True  # False once a scanned range reported an error
        self.avg_bytes = None

    def _snapshot(self, count_ptr: int, r: int) -> _Snapshot:
        """Block until everything launched so far has run; bring back the
        status words, the chain end, the running totals at row r and the
        word at count_ptr."""
        F = self.F if self.rows.planes is not None else 0
        n = 2 + _ST_CARRY + 3 * F
        buf = pinned_buffer("snapshot", n * 8)
        v, b, l = ([t.data_ptr() for t in self.rows.planes] if F
                   else (0, 0, 0))
        _native.gpu_stream_snapshot(
            count_ptr, self.status.addr(0), _ST_CARRY,
            self.status.carry_addr(self.nchain), v, b, l, self.rows.cap + 1,
            F, r, buf.data_ptr(), _stream())
        _native.gpu_stream_snapshot_wait()
        last_read["host_waits"] = last_read.get("host_waits", 0) + 1
        return _Snapshot(buf.numpy()[:n * 8].view(np.int64).copy(), F)

    def _settle(self, snap: _Snapshot):
        """What a snapshot at row r_done says about the launches before it:
        error words stop the extraction (they are raised at the end); a
        confirmed extraction advances x_done; one the gate refused had totals
        beyond the buffers, which are now known: regrow."""
        crc_bad, rc, _ = snap.scan_error
        if crc_bad != -1 or rc != 0:
            self.clean = False
        if self.x_pending is None:
            return
        assert self.x_pending == self.r_done
        if not snap.refused:
            self.x_done = self.x_pending
            self.vals.confirm(snap.totals)
        elif self.clean:
            self.vals.reserve(snap.totals, self.bytes_done)
        self.x_pending = None

    def _extract(self, r1: int, gated: bool):
        st = self.status
        gate = (st.addr(_ST_BROKEN), st.addr(_ST_CRC), st.addr(_ST_ERR),
                st.addr(_ST_NOEXT)) if gated else None
        self.vals.extract(self.data, self.rows.stats, self.rows.planes,
                          self.rows.presence, self.x_done, r1, self.meta,
                          st.xerr, self.avg_bytes, gate)

    def step(self, p: stream_plan.SlicePlan, counts: Optional[torch.Tensor],
             last: bool) -> bool:
        """Slice p has landed and `counts` holds its per-block candidate
        counts (None: nothing to scan). False when the chain broke."""
        count_ptr = 0
        if counts is not None:
            block_off = excl_sum(counts)
            count_ptr = block_off.data_ptr() + counts.numel() * 8
        # the one blocking wait of the slice; later slices are in flight
        snap = self._snapshot(count_ptr, self.r_done)
        if snap.broken:
            return False
        if self.do_scan:
            self._settle(snap)
        c_s = snap.count
        if c_s:
            # discovery: make room, EMIT the candidates behind the earlier
            # ones and chain them on from the previous launch's end
            self.rows.reserve(self.C + c_s, self.C, self.r_done, p.scan_hi)
            pos, lens, off = self.rows.cand_ptrs(self.C)
            _native.gpu_frame_scan_emit(self.data.data_ptr(), self.n,
                                        p.scan_lo, p.scan_hi, 0,
                                        block_off.data_ptr(), pos, lens,
                                        _stream())
            _native.gpu_frame_chain(pos, lens, c_s,
                                    self.status.carry_addr(self.nchain),
                                    self.status.carry_addr(self.nchain + 1),
                                    off, self.status.addr(_ST_BROKEN),
                                    _stream())
            self.nchain += 1
            self.C += c_s
        if not self.do_scan:
            return True
        # Before the last slice the last chained candidate always waits: in
        # an unbroken chain every other one ends where its successor starts,
        # below scan_hi, so it has arrived. After the last slice every
        # candidate has (they end inside the file: the COUNT cull).
        avail = stream_plan.launchable_records(self.C, last)
        r0 = self.r_done
        if avail > r0:
            if self.avg_bytes is None:  # wave/lane choice: once per file
                self.avg_bytes = max(0, p.scan_hi // avail - 16)
            off, lens, stats = self.rows.row_ptrs(r0)
            _native.gpu_scan_records(
                self.data.data_ptr(), off, lens, avail - r0,
                FMT[self.record_type], self.blob.data_ptr(), self.F, stats,
                self.status.err.data_ptr(),
                self.status.addr(_ST_CRC) if self.verify_crc else 0, _stream(),
                self.avg_bytes, rec_base=r0,
                gate=self.status.addr(_ST_BROKEN))
            self.rows.scan_stats(r0, avail)
            self.r_done = avail
        self.bytes_done = p.scan_hi
        if not _STREAM_EXTRACT or not self.clean or avail <= self.x_done:
            return True
        if not self.sized:
            if last:
                return True  # finish() sizes exactly
            # The first extraction sizes every value buffer from measured
            # density: one more wait, under the later slices' copies. From
            # here on extraction is optimistic and the gate catches a jump.
            snap = self._snapshot(0, avail)
            if snap.broken:
                return False
            self._settle(snap)
            if not self.clean:
                return True
            self.vals.reserve(snap.totals, p.scan_hi)
            self.sized = True
        self._extract(avail, gated=True)
        self.x_pending = avail
        return True

    def finish(self) -> Optional[RecordBatch]:
        """After the last slice: the final snapshot, the errors in
        decode_device's order, the rows not yet extracted, the columns. None
        when the chain did not hold over the whole file."""
        R, n = self.C, self.n
        if R == 0:
            return None
        snap = self._snapshot(0, R)
        if snap.broken or snap.chain_end != n:
            return None
        if not self.do_scan:
            return decode_device(self.data, self.rows.off[:R],
                                 self.rows.lens[:R], self.schema,
                                 self.record_type, self.verify_crc)
        crc_bad, rc, rec1 = snap.scan_error
        _raise_scan_errors(crc_bad if self.verify_crc else -1, rc, rec1)
        if not self.clean:
            raise RuntimeError("streamed decode: scan error lost")
        self._settle(snap)
        xerr = snap.xerr
        if self.x_done < R:
            # not streamed, or the gate refused the last launch: every total
            # is known now, so size exactly and extract (the rare path)
            self.vals.reserve(snap.totals, n)
            self._extract(R, gated=False)
            self.x_done = R
            self.vals.confirm(snap.totals)
            xerr = self._snapshot(0, R).xerr
        val_base, _, list_base = self.rows.planes
        cols = self.vals.columns(self.rows.presence, val_base, list_base, R)
        if xerr[0] != 0:
            _raise_extract_error(*xerr)
        return RecordBatch(self.schema, cols, R)


def _issue_h2d_slices(data: torch.Tensor, ptr: int, plan) -> list:
    """Issue ALL H2D slices up front on the side streams. Returns one list
    of events per slice: the main stream gates each slice's work on just
    that slice's copies."""
    main = torch.cuda.current_stream()
    streams = _dma_streams()
    for st in streams:
        st.wait_stream(main)  # `data` allocation ordering
    events = []
    for s, p in enumerate(plan):
        # each slice goes half on either DMA stream: the streams share the
        # link, so whole slices alternating between them land in PAIRS;
        # split, slice k lands alone while k+1 is still in flight
        half = (p.b1 - p.b0) // 2 if _SPLIT_SLICES and len(streams) > 1 else 0
        parts = ([(p.b0, p.b0 + half, 0), (p.b0 + half, p.b1, 1)] if half
                 else [(p.b0, p.b1, s % len(streams))])
        evs = []
        for lo, hi, k in parts:
            st = streams[k]
            _native.gpu_memcpy_h2d(data.data_ptr() + lo, ptr + lo, hi - lo,
                                   st.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(st)
            evs.append(ev)
        events.append(evs)
    for st in streams:
        data.record_stream(st)
    return events


def _scan_blocks(p: stream_plan.SlicePlan) -> int:
    """Frame-scan blocks (== block_counts entries) of slice p's scan range."""
    if p.scan_hi <= p.scan_lo:
        return 0
    return int(_native.gpu_frame_scan_blocks(p.scan_lo, p.scan_hi))


def _count_slice(data, p, evs, block_counts, base: int) -> int:
    """Once slice p's copies (events evs) have landed: the COUNT pass over
    its scan range into block_counts[base:]. Returns its block count."""
    main = torch.cuda.current_stream()
    for ev in evs:
        main.wait_event(ev)
    nb = _scan_blocks(p)
    if nb:
        _native.gpu_frame_scan_count(data.data_ptr(), data.numel(), p.scan_lo,
                                     p.scan_hi, base, block_counts.data_ptr(),
                                     _stream())
    return nb


def _read_unstreamed(data, plan, block_counts, events, first: int,
                     schema: StructType, record_type: str,
                     verify_crc: bool) -> RecordBatch:
    """The unstreamed read: COUNT under the DMA for the slices from `first`
    on (the earlier ones have been counted), then the whole-file
    _emit_and_chain + decode_device. TFREC_STREAM_DECODE=0 starts here with
    first == 0; the streamed loop leaves through here on a broken chain."""
    last_read["path"] = "fallback" if _STREAM_DECODE else "unstreamed"
    base = sum(_scan_blocks(p) for p in plan[:first])
    for p, evs in zip(plan[first:], events[first:]):
        base += _count_slice(data, p, evs, block_counts, base)
    ranges = [(p.scan_lo, p.scan_hi) for p in plan if p.scan_hi > p.scan_lo]
    off, lens, _ = _emit_and_chain(data, ranges, block_counts, data.numel())
    return decode_device(data, off, lens, schema, record_type, verify_crc)


def read_file_to_batch_pipelined(path: str, schema: StructType, record_type: str,
                                 verify_crc: bool = True,
                                 device="cuda") -> RecordBatch:
    """File -> device batch with the H2D DMA sliced so the work on slice k
    runs while slice k+1 is still in flight: frame discovery (COUNT, prefix
    sum, EMIT), the chain check, the fused structure scan + CRC, the stat
    prefix sums and the extraction of the records that have fully arrived,
    with one blocking snapshot per slice (_StreamedRead.step).
    Positions within 32 bytes of a slice boundary are deferred to the next
    slice's launch (their load window extends past the boundary). After the
    last slice only that slice's work remains. A broken frame chain abandons
    the streamed attempt for _read_unstreamed, which is also what
    TFREC_STREAM_DECODE=0 runs."""
    check_native()
    n = os.path.getsize(path)
    if n == 0:
        z = torch.zeros(0, dtype=torch.int64, device=device)
        return decode_device(torch.zeros(0, dtype=torch.uint8, device=device),
                             z, z.clone(), schema, record_type, verify_crc)
    ptr, pinned = _native.file_mmap_pinned(path, n, False)
    if not pinned:
        data = _read_file_staged(path, torch.empty(n, dtype=torch.uint8,
                                                   device=device))
        off, lens = scan_frames_device(data)
        return decode_device(data, off, lens, schema, record_type, verify_crc)
    data = torch.empty(n, dtype=torch.uint8, device=device)
    plan = stream_plan.plan_slices(n, _READ_SLICE)
    S = len(plan)
    # pre-size the per-block count buffer over the slice scan ranges
    block_counts = torch.empty(max(sum(_scan_blocks(p) for p in plan), 1),
                               dtype=torch.int64, device=data.device)
    events = _issue_h2d_slices(data, ptr, plan)
    last_read.update(path="streamed", slices=S, regrows=0, host_waits=0)
    unstreamed = (data, plan, block_counts, events)
    decode = (schema, record_type, verify_crc)
    if not _STREAM_DECODE:
        return _read_unstreamed(*unstreamed, 0, *decode)

    rd = _StreamedRead(data, S, *decode)
    base = 0  # block_counts offset of the current slice
    for s, p in enumerate(plan):
        nb = _count_slice(data, p, events[s], block_counts, base)
        counts = block_counts[base:base + nb] if nb else None
        base += nb
        if not rd.step(p, counts, last=s == S - 1):
            return _read_unstreamed(*unstreamed, s + 1, *decode)
    batch = rd.finish()
    if batch is None:
        return _read_unstreamed(*unstreamed, S, *decode)
    return batch


def gz_device_meta(path: str):
    """Segment table of OUR gzip files (None for foreign/table-less gzip):
    gates the device-inflate read path."""
    from ..io import paths as P

    if not getattr(_native, "HAS_GPU_KERNELS", False):
        return None
    return P.parse_gz_segments_file(path)


def _device_inflate_group(data: torch.Tensor, gz_items, device) -> bool:
    """Inflate several gzip files' full-flush segments in one kernel launch
    per kernel shape (one segment per wave or per half-wave,
    csrc/hip/inflate.hip), each file's output landing
    at its slice of `data`. gz_items = [(path, parse_gz_segments_file meta,
    out_base)]. Compressed bodies DMA straight from the page cache (pinned
    mmaps). Returns False when the kernel reported any malformed segment —
    the caller redoes those files on host zlib. The gzip CRC32 trailer is
    NOT checked here: the TFRecord layer CRC32C-verifies every record of the
    inflated bytes (a corrupt stream also breaks the frame chain)."""
    comp, comp_offs, _ = _upload_group(gz_items, device)
    in_off = []
    in_len = []
    out_off = []
    out_len = []
    for (p, meta, out_base), coff in zip(gz_items, comp_offs):
        body_off, segs, _crc, _isize = meta
        so = coff + body_off
        uo = out_base
        for c, u in segs:
            in_off.append(so)
            in_len.append(c)
            out_off.append(uo)
            out_len.append(u)
            so += c
            uo += u
    # Route each segment to the kernel shape its data favors (measured,
    # profiles/RESULTS.md): literal-heavy segments — compression ratio near
    # 1, every output byte is one Huffman symbol — run ~20% faster TWO per
    # wave (half-wave streams share the same vector instructions); match-
    # heavy segments favor the whole-wave kernel (wide cooperative copies,
    # no divergence between halves). TFREC_INFLATE_STREAMS=1|2 forces one.
    meta_np = np.array([in_off, in_len, out_off, out_len], np.int64)
    force = os.environ.get("TFREC_INFLATE_STREAMS", "")
    spw_lit = 2
    if force in ("1", "2", "4"):
        spw_lit = int(force)
        lit = np.full(meta_np.shape[1], spw_lit > 1)
    else:
        lit = meta_np[1] >= (0.85 * np.maximum(meta_np[3], 1))
    err = torch.full((1,), -1, dtype=torch.int64, device=device)
    for mask, spw in ((lit, spw_lit), (~lit, 1)):
        k = int(mask.sum())
        if k == 0:
            continue
        idx = np.nonzero(mask)[0]
        if spw == 2 and k > 2:
            # pair like-sized segments in one wave: halves reconverge at
            # segment end, so a short partner idles under a long one
            idx = idx[np.argsort(-meta_np[3, idx], kind="stable")]
        sub = torch.as_tensor(
            np.ascontiguousarray(meta_np[:, idx])).to(device)
        _native.gpu_inflate_segments(
            comp.data_ptr(), sub[0].data_ptr(), sub[1].data_ptr(),
            sub[2].data_ptr(), sub[3].data_ptr(), k,
            data.data_ptr(), err.data_ptr(), _stream(), spw)
    return int(err.item()) == -1


class DeviceDecompressRejected(Exception):
    """A device decompressor refused some files of a group (`paths`); the
    caller reads those through the host codec and redoes the group without
    them."""

    def __init__(self, paths, message):
        super().__init__(message)
        self.paths = list(paths)


class ForeignGzipRejected(DeviceDecompressRejected):
    """The device inflater refused some table-less gzip files of a group
    (`paths`); the caller reads those through host zlib and redoes the
    group without them."""

    def __init__(self, paths):
        super().__init__(
            paths, f"device inflate rejected {len(paths)} gzip file(s)")


class SnappyRejected(DeviceDecompressRejected):
    """The device Snappy decoder refused a chunk of some `.snappy` files of
    a group (`paths`); the caller reads those on the host."""

    def __init__(self, paths):
        super().__init__(
            paths, f"device snappy decode rejected {len(paths)} file(s)")


# what the last foreign-gzip inflate did, per file: [(path, live chunks,
# marker symbols, error word)] — read by the tests and bench_suite.py
last_foreign: list = []

_FOREIGN_DEFAULT_CHUNK = 32 << 10
_FOREIGN_MAX_FILES = 4096  # per launch (the CRC kernel's grid.y)


def _foreign_chunk_bytes(chunk_bytes: Optional[int] = None) -> int:
    """Compressed bytes per speculative chunk: the argument, else
    TFREC_GZ_FOREIGN_CHUNK, else 32 KiB (zlib's level-6 blocks are about
    that long compressed, so a finer stride finds no more block starts)."""
    if chunk_bytes is None:
        chunk_bytes = os.environ.get("TFREC_GZ_FOREIGN_CHUNK",
                                     _FOREIGN_DEFAULT_CHUNK)
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < 64:
        raise ValueError(
            f"foreign gzip chunk stride must be >= 64 bytes, got {chunk_bytes}")
    return chunk_bytes


def foreign_gz_meta(path: str):
    """(body_off, body_len, crc32, isize) of a gzip file from its header and
    trailer alone, walking FEXTRA, FNAME, FCOMMENT and FHCRC (RFC 1952), or
    None when the file is not for the device's speculative inflater: not
    CM=8, shorter than 18 bytes, ISIZE 0, or a body of 4 GiB or more. Says
    nothing about a segment table: gz_device_meta is asked first."""
    if not getattr(_native, "HAS_GPU_KERNELS", False):
        return None
    try:
        size = os.path.getsize(path)
        if size < 18:
            return None
        with open(path, "rb") as f:
            head = f.read(min(size, 128 << 10))  # FEXTRA <= 64 KiB + names
            f.seek(size - 8)
            trailer = f.read(8)
    except OSError:
        return None
    return _foreign_gz_parse(head, trailer, size)


def _foreign_gz_parse(head: bytes, trailer: bytes, size: int):
    if head[:3] != b"\x1f\x8b\x08" or head[3] & 0xE0:
        return None
    flg = head[3]
    pos = 10
    if flg & 0x04:
        if pos + 2 > len(head):
            return None
        pos += 2 + int.from_bytes(head[pos:pos + 2], "little")
    for bit in (0x08, 0x10):  # FNAME, FCOMMENT: zero-terminated
        if flg & bit:
            end = head.find(b"\x00", pos)
            if end < 0:
                return None
            pos = end + 1
    if flg & 0x02:
        pos += 2
    body_len = size - 8 - pos
    crc = int.from_bytes(trailer[:4], "little")
    isize = int.from_bytes(trailer[4:], "little")
    # DEFLATE cannot expand past 1032:1: a larger ISIZE belongs to another
    # member or is damaged, and is not worth the buffers
    if (pos > len(head) or body_len <= 0 or body_len >= (1 << 32)
            or isize == 0 or isize > body_len * 1032 + 64):
        return None
    return pos, body_len, crc, isize


def _device_inflate_foreign_group(data: torch.Tensor, items, device,
                                  chunk_bytes: Optional[int] = None):
    """Inflate table-less gzip files in HBM by block-parallel speculative
    decode (csrc/hip/inflate_foreign.hip; the steps are laid out in
    csrc/inflate_spec_core.h). items = [(path, foreign_gz_meta, out_base)];
    each file's bytes land at data[out_base : out_base + isize]. All files
    share every launch, the compressed bodies DMA from the page cache, and
    the host waits once, for the per-file result words. The member CRC-32
    is always checked: acceptance rests on a speculative chain, so nothing
    but the checksum vouches for the bytes. Returns one bool per item;
    False = refused (the slice's content is unspecified), read the file
    through host zlib."""
    chunk = _foreign_chunk_bytes(chunk_bytes)
    CC, FC, RC = (_native.FOREIGN_CHUNK_COLS, _native.FOREIGN_FILE_COLS,
                  _native.FOREIGN_RES_COLS)
    piece = int(_native.FOREIGN_CRC_PIECE)
    ok_all = []
    del last_foreign[:]
    for lo in range(0, len(items), _FOREIGN_MAX_FILES):
        part = items[lo:lo + _FOREIGN_MAX_FILES]
        nfile = len(part)
        comp, comp_offs, comp_sizes = _upload_group(part, device)
        ft = np.zeros((nfile, FC), np.int64)
        chunk0 = sym0 = piece0 = 0
        for k, (p, meta, out_base) in enumerate(part):
            body_off, body_len, crc, isize = meta
            if (body_off + body_len + 8 != comp_sizes[k] or out_base < 0
                    or out_base + isize > data.numel()):
                raise ValueError(f"foreign gzip extents changed under the "
                                 f"read: {p}")
            nchunk = -(-body_len // chunk)
            ft[k, :9] = (comp_offs[k] + body_off, body_len, isize, crc, chunk0,
                         nchunk, out_base, sym0, piece0)
            chunk0 += nchunk
            sym0 += isize
            piece0 += -(-isize // piece)
        # chunk table rows: file, start -1, len 0, end 0, next -2 (none),
        # rc 0, out_off -1 (not live), live-list slot
        ct = np.zeros((chunk0, CC), np.int64)
        ct[:, 0] = np.repeat(np.arange(nfile), ft[:, 5])
        ct[:, 1] = -1
        ct[:, 4] = -2
        ct[:, 6] = -1
        res = np.zeros((nfile, RC), np.int64)
        res[:, 0] = -1
        ft_d = torch.as_tensor(ft).to(device)
        ct_d = torch.as_tensor(ct).to(device)
        res_d = torch.as_tensor(res).to(device)
        sym = torch.empty(sym0, dtype=torch.int16, device=device)
        piece_crc = torch.empty(piece0, dtype=torch.int32, device=device)
        max_pieces = int((-(-ft[:, 2] // piece)).max())
        _native.gpu_inflate_foreign(
            comp.data_ptr(), ft_d.data_ptr(), ct_d.data_ptr(),
            res_d.data_ptr(), piece_crc.data_ptr(), sym.data_ptr(),
            data.data_ptr(), nfile, chunk0, max_pieces, chunk, _stream())
        out = res_d.cpu().numpy()  # the one host wait
        for k, (p, _, _) in enumerate(part):
            ok_all.append(int(out[k, 0]) == -1)
            last_foreign.append((p, int(out[k, 1]), int(out[k, 3]),
                                 int(out[k, 0])))
    return ok_all


# what the last device Snappy decode did, per file: [(path, chunks, error
# word)] — read by the tests and bench_suite.py
last_snappy: list = []

# Largest raw chunk the device takes. One wave walks one chunk's elements
# serially, so a long chunk holds one wave while the rest of the card
# idles; 1 MiB covers Hadoop's default 256 KiB buffer (and four times it)
# and keeps the slowest wave's walk in the low milliseconds. A file with a
# longer chunk is read on the host.
SNAPPY_MAX_CHUNK_RAW = 1 << 20


def snappy_on_device() -> bool:
    """TFREC_SNAPPY=device|host: where GPU-engine reads decompress
    `.snappy` files (default device; host = pyarrow's Snappy)."""
    val = os.environ.get("TFREC_SNAPPY", "device").lower()
    if val not in ("device", "host"):
        raise ValueError(
            f"Unsupported TFREC_SNAPPY {val!r} (expected 'device' or 'host')")
    return val == "device"


def snappy_device_meta(path: str):
    """(chunk extents, total raw size) of a `.snappy` file from its block
    headers alone (io/paths.py snappy_walk over a read-only mmap: 8 header
    bytes and a length preamble per block, the bodies stay untouched), or
    None when the file is not for the device decoder: TFREC_SNAPPY=host, a
    malformed container, or a chunk above SNAPPY_MAX_CHUNK_RAW. The
    extents are an int64 array of rows (in_off, in_len, out_off, out_len).
    Gates the device read path; None sends the file to the host."""
    import mmap

    from ..io import paths as P

    if not getattr(_native, "HAS_GPU_KERNELS", False) or not snappy_on_device():
        return None
    try:
        size = os.path.getsize(path)
        if size == 0:
            return np.zeros((0, 4), np.int64), 0
        with open(path, "rb") as f:
            with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                chunks, total = P.snappy_walk(mm, path)
    except (OSError, ValueError):
        return None
    ext = np.array(chunks, np.int64).reshape(-1, 4)
    if ext.shape[0] and int(ext[:, 3].max()) > SNAPPY_MAX_CHUNK_RAW:
        return None
    return ext, total


def _snappy_max_waves(device) -> int:
    """Grid cap of the Snappy launch, in waves: 16 per CU. The kernel is
    bound by the latency of each element's copy, not by bandwidth, so more
    resident waves are more throughput: 1M flagship rows (3288 chunks) took
    5.75 ms at 8 per CU (two rounds of the grid-stride loop) and 3.61 ms at
    16, 24 or 28, where every chunk has a wave (profiles/RESULTS.md). More
    chunks than the cap take the kernel's grid-stride loop."""
    return 16 * torch.cuda.get_device_properties(device).multi_processor_count


def _device_unsnap_group(data: torch.Tensor, items, device):
    """Decode several `.snappy` files in HBM in ONE launch, one raw chunk
    per wave (csrc/hip/snappy.hip), each file's bytes landing at
    data[out_base : out_base + total]. items = [(path, snappy_device_meta,
    out_base)]. The compressed files DMA from the page cache (pinned mmaps)
    on the side streams, the chunk table is checked against both buffers
    here before it is uploaded, and the host waits once, for the per-file
    error words. Returns one bool per item; False = a chunk was refused
    (the slice's content is unspecified), read the file on the host."""
    del last_snappy[:]
    nfile = len(items)
    comp, comp_offs, comp_sizes = _upload_group(items, device)
    tables = []
    chunk0 = np.zeros(nfile, np.int64)
    nchunk = 0
    for k, (p, meta, out_base) in enumerate(items):
        ext, total = meta
        chunk0[k] = nchunk
        if ext.shape[0]:
            t = np.empty((ext.shape[0], 5), np.int64)
            t[:, 0] = ext[:, 0] + comp_offs[k]
            t[:, 1] = ext[:, 1]
            t[:, 2] = ext[:, 2] + out_base
            t[:, 3] = ext[:, 3]
            t[:, 4] = k
            # every extent inside its own file's slice of both buffers
            if (ext[:, 0].min() < 0 or ext[:, 1].min() < 0
                    or (ext[:, 0] + ext[:, 1]).max() > comp_sizes[k]
                    or ext[:, 2].min() < 0 or ext[:, 3].min() < 0
                    or (ext[:, 2] + ext[:, 3]).max() > total
                    or out_base < 0 or out_base + total > data.numel()):
                raise ValueError(f"snappy extents changed under the read: {p}")
            tables.append(t)
            nchunk += ext.shape[0]
    err = np.full(nfile, -1, np.int64)
    if nchunk:
        assert int(_native.SNAPPY_CHUNK_COLS) == 5
        ct_d = torch.as_tensor(np.concatenate(tables)).to(device)
        c0_d = torch.as_tensor(chunk0).to(device)
        err_d = torch.as_tensor(err).to(device)
        _native.gpu_unsnap_chunks(
            comp.data_ptr(), ct_d.data_ptr(), c0_d.data_ptr(), nchunk,
            data.data_ptr(), err_d.data_ptr(), _snappy_max_waves(device),
            _stream())
        err = err_d.cpu().numpy()  # the one host wait
    ok = []
    for k, (p, meta, _) in enumerate(items):
        ok.append(int(err[k]) == -1)
        last_snappy.append((p, int(meta[0].shape[0]), int(err[k])))
    return ok


class DeviceSource(NamedTuple):
    """Where a file's bytes come from when the device takes it."""
    kind: str    # "raw" | "gzip" | "foreign" | "snappy"
    meta: object  # what the kind's *_meta function returned; None for raw
    nbytes: int  # decompressed length


def _gzip_source(path: str) -> Optional[DeviceSource]:
    meta = gz_device_meta(path)
    if meta is None:
        return None
    return DeviceSource("gzip", meta, sum(u for _, u in meta[1]))


def _foreign_source(path: str) -> Optional[DeviceSource]:
    meta = foreign_gz_meta(path)
    return None if meta is None else DeviceSource("foreign", meta, meta[3])


def _snappy_source(path: str) -> Optional[DeviceSource]:
    meta = snappy_device_meta(path)
    return None if meta is None else DeviceSource("snappy", meta, meta[1])


def device_source(path: str,
                  foreign_gzip: bool = False) -> Optional[DeviceSource]:
    """THE place that decides where a file's bytes come from: a raw DMA,
    the segment-table inflater (our gzip), the speculative inflater (any
    other writer's gzip, only with `foreign_gzip`, and only after the
    segment table was looked for), the Snappy decoder, or, None, the host
    codec. Every read path asks here, once per file, and hands the answer
    on (read_files_to_batch `sources=`), so a file's header is walked once
    per read."""
    from ..io import paths as P

    codec = P.codec_from_path(path)
    if codec is None:
        return DeviceSource("raw", None, os.path.getsize(path))
    if codec == "gzip":
        return _gzip_source(path) or (_foreign_source(path) if foreign_gzip
                                      else None)
    if codec == "snappy":
        return _snappy_source(path)
    return None


def _source_image(path: str, src: Optional[DeviceSource], device,
                  chunk_bytes: Optional[int] = None) -> Optional[torch.Tensor]:
    """The bytes of one file in HBM, through the decoder `src` names. None
    when there is no source or the decoder refused the file (callers fall
    back to the host codec)."""
    if src is None:
        return None
    if src.kind == "raw":
        return read_file_to_device(path, device)
    data = torch.empty(max(src.nbytes, 1), dtype=torch.uint8,
                       device=device)[:src.nbytes]
    items = [(path, src.meta, 0)]
    if src.kind == "gzip":
        ok = _device_inflate_group(data, items, device)
    elif src.kind == "foreign":
        ok = _device_inflate_foreign_group(data, items, device, chunk_bytes)[0]
    else:
        ok = _device_unsnap_group(data, items, device)[0]
    return data if ok else None


def read_file_image(path: str, foreign_gzip: bool = False,
                    device="cuda") -> Optional[torch.Tensor]:
    """Any file device_source accepts -> its (decompressed) bytes in HBM.
    None when the file is for the host or the device refused it."""
    return _source_image(path, device_source(path, foreign_gzip), device)


def read_gzip_file_to_device(path: str, device="cuda") -> Optional[torch.Tensor]:
    """Our-format gzip file -> decompressed bytes in HBM via the device
    inflater. None when the file carries no segment table or the kernel
    rejected a segment (callers fall back to host zlib)."""
    return _source_image(path, _gzip_source(path), device)


def read_foreign_gzip_file_to_device(path: str,
                                     chunk_bytes: Optional[int] = None,
                                     device="cuda") -> Optional[torch.Tensor]:
    """Any single-member gzip file -> decompressed bytes in HBM via the
    speculative device inflater, CRC-32 checked. None when the file is not
    eligible (foreign_gz_meta) or the inflater refused it: multi-member,
    truncated, corrupt, CRC or ISIZE mismatch (callers fall back to host
    zlib)."""
    check_native()
    return _source_image(path, _foreign_source(path), device, chunk_bytes)


def read_snappy_file_to_device(path: str,
                               device="cuda") -> Optional[torch.Tensor]:
    """`.snappy` file -> decompressed bytes in HBM via the device decoder.
    None when the file is not eligible (snappy_device_meta) or the kernel
    refused a chunk (callers fall back to the host codec)."""
    check_native()
    return _source_image(path, _snappy_source(path), device)


def _deflate_max_waves(device) -> int:
    """Resident-wave cap of the compressor launch: its token workspace is
    sized per resident wave (4 B per input byte of one segment), not per
    segment. 78 KiB of LDS per 4-wave block fits two blocks per CU."""
    return 8 * torch.cuda.get_device_properties(device).multi_processor_count


def gzip_image_device(img: torch.Tensor, seg: Optional[int] = None) -> torch.Tensor:
    """Uncompressed file image in HBM -> complete gzip file image in HBM, in
    the layout io/paths.py compress_bytes writes (FEXTRA 'TS' segment
    table, independent full-flush segments, CRC-32/ISIZE trailer), via the
    device compressor (csrc/hip/deflate.hip). The layout is known up front,
    so the only host round trip is one read of the final image size."""
    from ..io import paths as P

    check_native()
    if img.dtype != torch.uint8 or img.dim() != 1 or not img.is_contiguous():
        raise ValueError("gzip_image_device expects a contiguous 1-D uint8 tensor")
    n = img.numel()
    if seg is None:
        seg = P._gz_segment_size(n)
    seg = int(seg)
    if seg <= 0:
        raise ValueError(f"segment size must be positive, got {seg}")
    nseg = max(1, -(-n // seg))
    if nseg > P._GZ_MAX_SEGS:
        raise ValueError(
            f"{n} bytes in {seg}-byte segments need {nseg} segments; the "
            f"gzip segment table holds at most {P._GZ_MAX_SEGS}")
    device = img.device
    seg_max = min(seg, n)
    slot = (_native.deflate_seg_out_bound(seg_max) + 7) & ~7
    nwaves = min(-(-nseg // 4) * 4, _deflate_max_waves(device))
    tok_cap = max(seg_max, 1)
    staging = torch.empty(nseg * slot, dtype=torch.uint8, device=device)
    tok_ws = torch.empty(nwaves * tok_cap, dtype=torch.int32, device=device)
    comp_len = torch.empty(nseg, dtype=torch.int64, device=device)
    comp_off = torch.empty(nseg + 1, dtype=torch.int64, device=device)
    seg_crc = torch.empty(nseg, dtype=torch.int32, device=device)
    err = torch.full((1,), -1, dtype=torch.int64, device=device)
    result = torch.empty(2, dtype=torch.int64, device=device)
    body_off = 20 + 8 * nseg
    out_cap = body_off + nseg * slot + 8
    out = torch.empty(out_cap, dtype=torch.uint8, device=device)
    _native.gpu_deflate_segments(
        img.data_ptr(), n, seg, nseg, staging.data_ptr(), slot,
        comp_len.data_ptr(), seg_crc.data_ptr(), tok_ws.data_ptr(), tok_cap,
        nwaves, float(P._GZ_STORED_THRESHOLD), err.data_ptr(), _stream())
    _excl_sum_into(comp_off.data_ptr(), comp_len.data_ptr(), 1, nseg, device)
    _native.gpu_gzip_assemble(
        staging.data_ptr(), slot, comp_len.data_ptr(), comp_off.data_ptr(),
        seg_crc.data_ptr(), n, seg, nseg, out.data_ptr(), out_cap,
        err.data_ptr(), result.data_ptr(), _stream())
    size, err_word = (int(v) for v in result.tolist())
    if err_word != -1:
        raise RuntimeError(
            f"device deflate failed: segment {(err_word >> 8) - 1}, "
            f"cause {err_word & 0xFF}")
    return out[:size]


def _snap_max_waves(device) -> int:
    """Resident-wave cap of the Snappy compressor launch, from the kernel's
    LDS use: a 4-wave block holds four 16 KiB hash tables (66 KiB with the
    window arrays), so two blocks fit a CU's 160 KiB. More blocks than
    waves take the kernel's grid-stride loop."""
    blocks_per_cu = max(1, (160 << 10) // int(_native.SNAP_LDS_BYTES_PER_BLOCK))
    return (int(_native.SNAP_WAVES_PER_BLOCK) * blocks_per_cu *
            torch.cuda.get_device_properties(device).multi_processor_count)


def snappy_image_device(img: torch.Tensor,
                        block: Optional[int] = None) -> torch.Tensor:
    """Uncompressed file image in HBM -> complete `.snappy` file image in
    HBM, in the layout io/paths.py snappy_walk describes (one raw chunk per
    block of `block` bytes), via the device compressor
    (csrc/hip/snappy_enc.hip). Every chunk's place follows from a scan of
    the chunk lengths on the device, so the only host round trip is one
    read of the final image size. An empty image is a zero-byte file."""
    from ..io import paths as P

    check_native()
    if img.dtype != torch.uint8 or img.dim() != 1 or not img.is_contiguous():
        raise ValueError(
            "snappy_image_device expects a contiguous 1-D uint8 tensor")
    if block is None:
        block = P.snappy_block_size()
    block = int(block)
    if block <= 0:
        raise ValueError(f"block size must be positive, got {block}")
    if block > SNAPPY_MAX_CHUNK_RAW:
        raise ValueError(
            f"block size {block} is above the device's {SNAPPY_MAX_CHUNK_RAW}"
            " bytes per chunk")
    n = img.numel()
    device = img.device
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=device)
    nblk = -(-n // block)
    slot = (_native.snappy_out_bound(min(block, n)) + 7) & ~7
    nwaves = min(-(-nblk // 4) * 4, _snap_max_waves(device))
    staging = torch.empty(nblk * slot, dtype=torch.uint8, device=device)
    comp_len = torch.empty(nblk, dtype=torch.int64, device=device)
    comp_off = torch.empty(nblk + 1, dtype=torch.int64, device=device)
    err = torch.full((1,), -1, dtype=torch.int64, device=device)
    result = torch.empty(2, dtype=torch.int64, device=device)
    # no chunk is longer than its block as one literal: n + 10 at the most
    out_cap = nblk * (8 + 10) + n
    out = torch.empty(out_cap, dtype=torch.uint8, device=device)
    _native.gpu_snap_blocks(
        img.data_ptr(), n, block, nblk, staging.data_ptr(), slot,
        comp_len.data_ptr(), nwaves, err.data_ptr(), _stream())
    _excl_sum_into(comp_off.data_ptr(), comp_len.data_ptr(), 1, nblk, device)
    _native.gpu_snappy_assemble(
        staging.data_ptr(), slot, comp_len.data_ptr(), comp_off.data_ptr(),
        n, block, nblk, out.data_ptr(), out_cap, err.data_ptr(),
        result.data_ptr(), _stream())
    size, err_word = (int(v) for v in result.tolist())
    if err_word != -1:
        raise RuntimeError(
            f"device snappy compress failed: block {(err_word >> 8) - 1}, "
            f"cause {err_word & 0xFF}")
    if size > out_cap:
        raise RuntimeError(
            f"device snappy compress: image of {size} bytes, room for {out_cap}")
    return out[:size]


def read_files_to_batch(paths, schema: StructType, record_type: str,
                        verify_crc: bool = True, device="cuda",
                        foreign_gzip: bool = False, sources=None):
    """Decode MANY files as ONE GPU pipeline: their (decompressed) images
    are concatenated in HBM (TFRecord frames are concatenable, so the frame
    chain spans file boundaries exactly), scanned and decoded once, and the
    per-file row counts recovered with a searchsorted over frame offsets.
    Uncompressed files DMA straight from the page cache; gzip files bearing
    our segment table are inflated by the device inflater (all files'
    segments in one launch); `.snappy` files are decoded by the device
    Snappy decoder (all files' chunks in one launch), and SnappyRejected
    names those it refuses. With `foreign_gzip`, gzip files without the
    table go through the speculative inflater into their own slices of the
    same image; if it refuses any, ForeignGzipRejected names them and
    nothing is decoded. `sources` hands over each path's device_source
    record where the caller already has it; without it the files are
    classified here. Returns (device RecordBatch, np.ndarray row_counts per
    file)."""
    from ..io import paths as P

    check_native()
    if sources is None:
        sources = [device_source(p, foreign_gzip) for p in paths]
    for p, src in zip(paths, sources):
        if src is None:
            what = {"gzip": "gzip file without segment table",
                    "snappy": "snappy file not for the device decoder"}
            raise ValueError(
                f"{what.get(P.codec_from_path(p), 'file not for the device')}"
                f": {p} (host path required)")
    sizes = [src.nbytes for src in sources]
    n = sum(sizes)
    if n == 0:
        if schema is None:
            raise ValueError(
                "Could not infer schema: no non-empty TFRecord files found")
        z = torch.zeros(0, dtype=torch.int64, device=device)
        return (decode_device(torch.zeros(0, dtype=torch.uint8, device=device),
                              z, z.clone(), schema, record_type, verify_crc),
                np.zeros(len(paths), np.int64))
    data = torch.empty(n, dtype=torch.uint8, device=device)
    bounds = np.zeros(len(paths) + 1, np.int64)
    np.cumsum(sizes, out=bounds[1:])
    # each non-empty file with its slice of the image, bucketed by kind
    raw_files = []
    items = {"gzip": [], "foreign": [], "snappy": []}
    for p, src, base in zip(paths, sources, bounds):
        if src.kind == "raw":
            raw_files.append((p, src.nbytes, int(base)))
        elif src.nbytes:
            items[src.kind].append((p, src.meta, int(base)))
    gz_items, foreign_items, snappy_items = (
        items["gzip"], items["foreign"], items["snappy"])
    _upload_files(data, raw_files)
    if foreign_items:
        ok = _device_inflate_foreign_group(data, foreign_items, device)
        refused = [it[0] for it, good in zip(foreign_items, ok) if not good]
        if refused:
            # a refused file's true length is unknown (its ISIZE may be
            # another member's), so the image layout cannot be kept
            raise ForeignGzipRejected(refused)
    if snappy_items:
        ok = _device_unsnap_group(data, snappy_items, device)
        refused = [it[0] for it, good in zip(snappy_items, ok) if not good]
        if refused:
            # the host decoder decides what a refused file is: its bytes,
            # or an error that names the file
            raise SnappyRejected(refused)
    if gz_items and not _device_inflate_group(data, gz_items, device):
        # rare fallback: a segment the kernel rejected — host zlib fills
        # the affected files' slices
        import logging

        logging.getLogger(__name__).warning(
            "device inflate rejected a segment; host zlib fallback for "
            "%d gzip file(s)", len(gz_items))
        for p, meta, base in gz_items:
            blob = np.frombuffer(P.decompress_file(p), np.uint8)
            stage = pinned_buffer("gzfb", blob.size)
            stage.numpy()[:blob.size] = blob
            data[base:base + blob.size].copy_(stage[:blob.size],
                                              non_blocking=True)
            # the staging buffer is reused next iteration: wait out the copy
            torch.cuda.current_stream().synchronize()
    off, lens = scan_frames_device(data)
    frame_start = off - 12
    counts = torch.searchsorted(
        frame_start, torch.as_tensor(bounds, device=device)).cpu().numpy()
    row_counts = np.diff(counts)
    if schema is None:
        # FUSED schema inference: the reference scans the first non-empty
        # file in a separate job (DefaultSource.scala:31-39); here the file
        # image is already in HBM, so the lattice kernel runs over that
        # file's frames and the decode reuses the same image — a
        # schema-less read costs ONE pass instead of two.
        from ..infer import byte_array_schema, schema_from_codes

        if record_type == "ByteArray":
            schema = byte_array_schema()
        else:
            i = next((k for k in range(len(paths)) if row_counts[k] > 0), None)
            if i is None:
                raise ValueError(
                    "Could not infer schema: no non-empty TFRecord files found")
            r0, r1 = int(counts[i]), int(counts[i + 1])
            codes = infer_codes_device(data, off[r0:r1].contiguous(),
                                       lens[r0:r1].contiguous(), record_type)
            schema = schema_from_codes(codes)
    batch = decode_device(data, off, lens, schema, record_type, verify_crc)
    return batch, row_counts


def encode_partitions_device(batch: RecordBatch, part_codes: np.ndarray,
                             num_parts: int, record_type: str):
    """Encode ALL rows once, then split into per-partition file images by
    GATHERING framed records (TFRecord frames are concatenable, so a
    partitioned write never re-serializes a row — the partition step is a
    pure byte gather in HBM). Returns (image, [(part_code, lo, hi), ...])
    where image[lo:hi] is partition part_code's complete file image.

    The reference delegates this grouping to Spark's FileFormatWriter sort
    (SURVEY.md §3.3); here the grouping is a device argsort of partition
    codes + one gather kernel pass."""
    check_native()
    R = batch.num_rows
    device = batch.columns[0].presence.device if batch.columns else torch.device("cuda")
    cols_dev, blob, psize, frame_off = _size_records(batch, record_type, device)
    total = int(frame_off[-1].item())
    file = torch.empty(total, dtype=torch.uint8, device=device)
    err = torch.zeros(2, dtype=torch.int32, device=device)
    _native.gpu_emit_records(cols_dev.data_ptr(), blob.data_ptr(),
                             FMT[record_type], 0, R, frame_off.data_ptr(),
                             file.data_ptr(), err.data_ptr(), _stream(),
                             total // max(R, 1))
    codes = torch.as_tensor(np.ascontiguousarray(part_codes, np.int64),
                            device=device)
    order = torch.argsort(codes, stable=True)
    sizes = psize[order].contiguous()
    dst_off = excl_sum(sizes)
    src_off = frame_off[:-1][order].contiguous()
    out = torch.empty(total, dtype=torch.uint8, device=device)
    _native.gpu_gather_payloads(file.data_ptr(), src_off.data_ptr(),
                                sizes.data_ptr(), dst_off.data_ptr(), R,
                                out.data_ptr(), _stream(), total // max(R, 1))
    # partition boundaries in the ordered space
    counts = torch.bincount(codes, minlength=num_parts)
    row_bound = torch.nn.functional.pad(torch.cumsum(counts, 0), (1, 0))
    byte_bound = dst_off[row_bound].cpu().numpy()
    _check_emit_err(err)
    ranges = [(p, int(byte_bound[p]), int(byte_bound[p + 1]))
              for p in range(num_parts) if byte_bound[p + 1] > byte_bound[p]]
    return out, ranges


# ---------------------------------------------------------------------------
# Schema inference on device: hash-table lattice kernel.
# ---------------------------------------------------------------------------

_INFER_SLOTS = 2048       # 1024 context + 1024 sequence feature names
_INFER_SLOTS_MAX = 1 << 21  # growth cap (1M distinct names per half)
_ERR_OVERFLOW = -5
_ERR_NAME_TOO_LONG = -6


def infer_codes_device(data: torch.Tensor, off: torch.Tensor,
                       lens: torch.Tensor, record_type: str) -> dict:
    """Device records -> {feature name: lattice code}. The kernel interns
    names into a device hash table and max-merges per-feature codes; the
    host only reads back the (tiny) table and resolves name strings. The
    table GROWS on overflow (datasets with thousands of distinct feature
    names rerun the kernel with 4x the slots; the scan is cheap relative to
    the decode it precedes, so the retry is simpler than spilling)."""
    check_native()
    device = data.device
    fmt = FMT["SequenceExample" if record_type == "SequenceExample" else "Example"]
    R = off.numel()
    slots = _INFER_SLOTS
    while True:
        table = torch.zeros((slots, 3), dtype=torch.int64, device=device)
        err = torch.zeros(2, dtype=torch.int32, device=device)
        if R:
            _native.gpu_infer_codes(data.data_ptr(), off.data_ptr(),
                                    lens.data_ptr(), R, fmt, table.data_ptr(),
                                    slots, err.data_ptr(), _stream())
        tab = table.cpu().numpy()
        rc = int(err[0].item())
        if rc == _ERR_OVERFLOW:
            if slots < _INFER_SLOTS_MAX:
                slots *= 4
                continue
            raise RuntimeError(
                "schema inference failed: more than "
                f"{_INFER_SLOTS_MAX // 2} distinct feature names")
        if rc == _ERR_NAME_TOO_LONG:
            raise RuntimeError(
                "schema inference failed: a feature name exceeds 65535 bytes")
        if rc != 0:
            rec = int(err[1].item()) - 1
            where = f" (record {rec})" if rec >= 0 else ""
            raise RuntimeError(f"malformed record during schema inference"
                               f"{where} (native error {rc})")
        break
    used = np.nonzero(tab[:, 0])[0]
    if len(used) == 0:
        return {}
    # recover name strings: one D2H of the covering range when it is small,
    # else one tiny D2H per distinct name (names are first occurrences and
    # can be anywhere in the file)
    refs = tab[used, 1]
    offs = (refs >> 16).astype(np.int64)
    nlens = (refs & 0xFFFF).astype(np.int64)
    lo = int(offs.min())
    hi = int((offs + nlens).max())
    codes: dict = {}
    if hi - lo <= (4 << 20):
        blob = data[lo:hi].cpu().numpy().tobytes()
        for o, ln, code in zip(offs, nlens, tab[used, 2]):
            name = blob[o - lo:o - lo + ln].decode("utf-8", errors="replace")
            codes[name] = max(codes.get(name, 0), int(code))
    else:
        for o, ln, code in zip(offs, nlens, tab[used, 2]):
            name = data[o:o + ln].cpu().numpy().tobytes().decode("utf-8", errors="replace")
            codes[name] = max(codes.get(name, 0), int(code))
    return codes


def infer_schema_file(path: str, record_type: str, device="cuda"):
    """Uncompressed file -> inferred StructType, fully on the GPU."""
    from ..infer import schema_from_codes

    data = read_file_to_device(path, device)
    off, lens = scan_frames_device(data)
    return schema_from_codes(infer_codes_device(data, off, lens, record_type))


def batch_to_device(batch: RecordBatch, device="cuda") -> RecordBatch:
    cols = []
    for c in batch.columns:
        cols.append(WireColumn(
            c.kind, c.is_seq,
            _dev(c.presence, torch.uint8, device),
            _dev(c.row_off, torch.int64, device),
            _dev(c.values, {KIND_INT64: torch.int64, KIND_FLOAT: torch.float32,
                            KIND_BYTES: torch.uint8}[c.kind], device),
            _dev(c.elem_off, torch.int64, device) if c.elem_off is not None else None,
            _dev(c.list_off, torch.int64, device) if c.list_off is not None else None,
            _dev(c.sub_off, torch.int64, device) if c.sub_off is not None else None,
        ))
    return RecordBatch(batch.schema, cols, batch.num_rows)


def batch_to_host(batch: RecordBatch) -> RecordBatch:
    """Device batch -> host numpy batch. All D2H copies go into PINNED
    host tensors (torch's caching host allocator reuses them) issued
    async round-robin over the TWO side streams with one sync at the end —
    pageable `.cpu()` per tensor runs at ~8 GB/s with a hidden staging
    copy, one pinned stream at ~35, two at link speed. The numpy arrays
    are zero-copy views of the pinned tensors (kept alive by the view's
    base)."""
    streams = _dma_streams()
    main = torch.cuda.current_stream()
    state = {"used": False, "k": 0}

    def h(t):
        if not isinstance(t, torch.Tensor):
            return t
        if not t.is_cuda:
            return t.numpy()
        host = torch.empty_like(t, device="cpu", pin_memory=True)
        if not state["used"]:
            for s in streams:
                s.wait_stream(main)
            state["used"] = True
        nbytes = t.numel() * t.element_size()
        if nbytes >= (8 << 20) and t.is_contiguous() and len(streams) > 1:
            # a single dominant tensor (ByteArray values, big value columns)
            # would ride ONE stream under round-robin and cap at the
            # single-blit rate (~21 GB/s measured); split it across both
            flat_d = t.view(-1)
            flat_h = host.view(-1)
            n = flat_d.numel()
            step = (n + len(streams) - 1) // len(streams)
            for i, st in enumerate(streams):
                lo = i * step
                hi = min(n, lo + step)
                if lo >= hi:
                    break
                with torch.cuda.stream(st):
                    flat_h[lo:hi].copy_(flat_d[lo:hi], non_blocking=True)
                t.record_stream(st)
            return host.numpy()
        st = streams[state["k"] % len(streams)]
        state["k"] += 1
        with torch.cuda.stream(st):
            host.copy_(t, non_blocking=True)
        t.record_stream(st)
        return host.numpy()

    cols = [WireColumn(c.kind, c.is_seq, h(c.presence), h(c.row_off), h(c.values),
                       h(c.elem_off) if c.elem_off is not None else None,
                       h(c.list_off) if c.list_off is not None else None,
                       h(c.sub_off) if c.sub_off is not None else None)
            for c in batch.columns]
    if state["used"]:
        for s in streams:
            s.synchronize()
    return RecordBatch(batch.schema, cols, batch.num_rows)


# ---------------------------------------------------------------------------
# CPU-boundary convenience wrappers (used by the file reader/writer)
# ---------------------------------------------------------------------------

def decode_buffer_to_cpu(data_np: np.ndarray, schema: StructType, record_type: str,
                         verify_crc: bool = True) -> RecordBatch:
    return batch_to_host(decode_buffer_device(data_np, schema, record_type,
                                              verify_crc))


def encode_batch_from_cpu(batch: RecordBatch, record_type: str) -> bytes:
    dev_batch = batch_to_device(batch)
    file = encode_device(dev_batch, record_type)
    return device_to_bytes(file)
