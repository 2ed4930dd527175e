"""Does compute on the main stream slow the sliced H2D of the pipelined reader?

The flagship file image (1M-row Example, ~215 MB) is read from its
registered mapping in _READ_SLICE slices on the two DMA streams, exactly as
read_file_to_batch_pipelined issues them. Variants, interleaved per round:

  h2d          the copies alone
  serial       the copies, then ONE fused scan+CRC launch over all records
  ovl@G        per slice, once its event fired, a fused scan+CRC launch over
               the records that have fully arrived; grid capped at G blocks
               (0 = the wrapper's own cap)

Per variant: time from the first copy's issue to the last copy's end (h2d)
and to the last kernel's end (end), median and min-max over the rounds.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import make_batch
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.columnar import schema_blob, wire_fields
from spark_tfrecord_amd.engine import gpu

ROWS = int(os.environ.get("ROWS", 1_000_000))
ROUNDS = int(os.environ.get("ROUNDS", 15))
GRIDS = [int(g) for g in os.environ.get("GRIDS", "0,1024,256").split(",")]

batch = make_batch(ROWS, seed=1234)
path = "/dev/shm/exp_overlap.tfrecord"
n = gpu.write_batch_to_file(gpu.batch_to_device(batch), path, "Example")
ptr, pinned = _native.file_mmap_pinned(path, n, False)
assert pinned, "needs a registered file mapping"

data = gpu.read_file_to_device(path)
off, lens = gpu.scan_frames_device(data)
R = off.numel()
ends = (off + lens + 4).cpu().numpy()  # record end incl. payload CRC
fields = wire_fields(batch.schema)
F = len(fields)
blob = torch.frombuffer(bytearray(schema_blob(batch.schema)),
                        dtype=torch.uint8).to("cuda")
stats = torch.empty((R, F, 6), dtype=torch.int64, device="cuda")
err = torch.zeros(2, dtype=torch.int32, device="cuda")
crc_err = torch.full((1,), -1, dtype=torch.int64, device="cuda")
avg = max(0, n // R - 16)

span = gpu._READ_SLICE
S = (n + span - 1) // span
# records fully arrived after slice s
K = [int(np.searchsorted(ends, min(n, (s + 1) * span), side="right"))
     for s in range(S)]
main = torch.cuda.current_stream()
streams = gpu._dma_streams()
dst = torch.empty(n, dtype=torch.uint8, device="cuda")


def scan(r0, r1, max_blocks):
    if r1 <= r0:
        return
    _native.gpu_scan_records(dst.data_ptr(), off.data_ptr() + r0 * 8,
                             lens.data_ptr() + r0 * 8, r1 - r0,
                             gpu.FMT["Example"], blob.data_ptr(), F,
                             stats.data_ptr() + r0 * F * 48, err.data_ptr(),
                             crc_err.data_ptr(), main.cuda_stream, avg,
                             rec_base=r0, max_blocks=max_blocks)


def run(mode, max_blocks=0):
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t_h2d = [torch.cuda.Event(enable_timing=True) for _ in streams]
    t_end = torch.cuda.Event(enable_timing=True)
    t0.record(main)
    for st in streams:
        st.wait_stream(main)
    events = []
    for s in range(S):
        b0, b1 = s * span, min(n, (s + 1) * span)
        st = streams[s % len(streams)]
        _native.gpu_memcpy_h2d(dst.data_ptr() + b0, ptr + b0, b1 - b0,
                               st.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(st)
        events.append(ev)
    for st, e in zip(streams, t_h2d):
        e.record(st)
    done = 0
    for s in range(S):
        main.wait_event(events[s])
        if mode == "ovl":
            scan(done, K[s], max_blocks)
            done = K[s]
    if mode == "serial":
        scan(0, R, 0)
    t_end.record(main)
    torch.cuda.synchronize()
    return max(t0.elapsed_time(e) for e in t_h2d), t0.elapsed_time(t_end)


variants = [("h2d", "h2d", 0), ("serial", "serial", 0)] + \
    [(f"ovl@{g}", "ovl", g) for g in GRIDS]
for _, mode, g in variants:  # warm
    run(mode, g)
res = {name: [] for name, _, _ in variants}
for _ in range(ROUNDS):
    for name, mode, g in variants:
        res[name].append(run(mode, g))
assert int(crc_err.item()) == -1 and int(err[0].item()) == 0

print(f"# {n / 1e6:.1f} MB, {R} records, {S} slices of {span >> 20} MiB, "
      f"{ROUNDS} rounds; ms from first copy issue")
print(f"{'variant':10s} {'h2d med':>8s} {'h2d min-max':>15s} "
      f"{'end med':>8s} {'end min-max':>15s}")
for name, _, _ in variants:
    a = np.asarray(res[name])
    print(f"{name:10s} {np.median(a[:, 0]):8.3f} "
          f"{a[:, 0].min():7.3f}-{a[:, 0].max():7.3f} "
          f"{np.median(a[:, 1]):8.3f} "
          f"{a[:, 1].min():7.3f}-{a[:, 1].max():7.3f}")
os.unlink(path)
