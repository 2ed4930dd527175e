#!/usr/bin/env python3
"""Host copy of the staged read, alone: GB/s of filling a pinned buffer from
the flagship file on tmpfs, (a) pread_parallel from the fd and (b)
memcpy_parallel from the file's cached mapping (the write has just stored
through it, so its pages are mapped), span by span at 2/4/8/32 MiB, with the
IO pool at each size in --pools (one child process per size; a size other
than the pool's own 8 needs a build whose IOPool reads TFREC_IO_THREADS,
which r13 had for this measurement and dropped after it). Needs a GPU (the file is
written by the GPU engine and the buffer is pinned); no device work is timed.

    python exp/exp_stage_source.py [--rows 1000000] [--pools 8] [--reps 9]
"""

import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPANS = [2 << 20, 4 << 20, 8 << 20, 32 << 20]


def child(rows: int, reps: int):
    import torch
    from bench import make_batch
    from spark_tfrecord_amd import _native
    from spark_tfrecord_amd.engine import gpu

    d = "/dev/shm/tfrec_exp_stage"
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "f.tfrecord")
    dev = gpu.batch_to_device(make_batch(rows, seed=1234))
    for _ in range(2):
        n = gpu.write_batch_to_file(dev, path, "Example")
    torch.cuda.synchronize()
    ptr, pinned = _native.file_mmap_pinned(path, n, False)
    buf = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    buf.zero_()  # fault the pinned pages in
    dst = buf.data_ptr()
    fd = os.open(path, os.O_RDONLY)
    pool = int(os.environ.get("TFREC_IO_THREADS", 8))
    print(json.dumps({"file_bytes": n, "mapping_registered": bool(pinned),
                      "mapping": bool(ptr), "pool": pool}), flush=True)

    def fill(source, span):
        for o in range(0, n, span):
            m = min(span, n - o)
            if source == "pread":
                _native.pread_parallel(fd, dst + o, m, o)
            else:
                _native.memcpy_parallel(dst + o, ptr + o, m)

    try:
        for source in ("pread", "map"):
            if source == "map" and not ptr:
                continue
            for span in SPANS:
                fill(source, span)  # warm
                ts = []
                for _ in range(reps):
                    t = time.perf_counter()
                    fill(source, span)
                    ts.append(time.perf_counter() - t)
                ts.sort()
                print(json.dumps({
                    "pool": pool, "source": source, "span_mib": span >> 20,
                    "ms_median": round(ts[len(ts) // 2] * 1e3, 3),
                    "ms_min": round(ts[0] * 1e3, 3),
                    "ms_max": round(ts[-1] * 1e3, 3),
                    "gbps_median": round(n / ts[len(ts) // 2] / 1e9, 2),
                    "gbps_best": round(n / ts[0] / 1e9, 2)}), flush=True)
        ok = bytes(buf[:4096].numpy()) == open(path, "rb").read(4096)
        print(json.dumps({"pool": pool, "bytes_check": ok}), flush=True)
    finally:
        os.close(fd)
        os.unlink(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--pools", type=str, default="8")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.rows, a.reps)
    for pool in a.pools.split(","):
        env = dict(os.environ, TFREC_IO_THREADS=pool)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child",
                        "--rows", str(a.rows), "--reps", str(a.reps)],
                       env=env, check=True, timeout=240)


if __name__ == "__main__":
    main()
