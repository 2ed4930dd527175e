#!/usr/bin/env python3
"""Where the streamed read's time goes, from a rocprofv3 trace.

    rocprofv3 --kernel-trace --memory-copy-trace --stats -d OUT -o t \\
        --output-format csv -- python bench.py --steps 3
    python exp/trace_tail.py OUT [--read N]

Reads every *kernel_trace.csv and *memory_copy_trace.csv below OUT. A read
is a run of large host-to-device copies (the file's slices); it ends where
the next write's first kernel (size_records) starts. Per read it prints the
copy landing times, the tail (last slice copy's end to the last decode
kernel's end) and the kernels that end after the last copy with their busy
time; for the chosen read (default: the last) also the kernel list from the
first copy's issue and, per slice, the wall time of the slice's kernel chain
(from its COUNT pass to the last kernel before the next COUNT pass) next to
the slice period (the distance between two landings).
"""

import argparse
import csv
import glob
import os

SLICE_COPY_MS = 0.1   # a slice copy takes longer than this, a table upload less
READ_GAP_MS = 2.0     # slice copies further apart belong to different reads
MIN_SLICE_COPIES = 4  # fewer: an input upload, not a sliced file read


def _rows(out_dir, suffix):
    rows = []
    for path in sorted(glob.glob(os.path.join(out_dir, "**", "*" + suffix),
                                 recursive=True)):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    return rows


def load(out_dir):
    kernels = [(int(r["Start_Timestamp"]) / 1e6, int(r["End_Timestamp"]) / 1e6,
                r["Kernel_Name"]) for r in _rows(out_dir, "kernel_trace.csv")]
    copies = [(int(r["Start_Timestamp"]) / 1e6, int(r["End_Timestamp"]) / 1e6,
               r.get("Direction", "")) for r in
              _rows(out_dir, "memory_copy_trace.csv")]
    return sorted(kernels), sorted(copies)


def find_reads(kernels, copies):
    """[(slice copies, decode kernels)] per read, times in ms."""
    big = [c for c in copies if "HOST_TO_DEVICE" in c[2]
           and c[1] - c[0] > SLICE_COPY_MS]
    groups = []
    for c in big:
        if groups and c[0] - groups[-1][-1][1] < READ_GAP_MS:
            groups[-1].append(c)
        else:
            groups.append([c])
    writes = [k[0] for k in kernels if "size_records" in k[2]]
    reads = []
    for i, g in enumerate(groups):
        t0 = g[0][0]
        t1 = min([w for w in writes if w > t0] +
                 [groups[i + 1][0][0] if i + 1 < len(groups) else float("inf")])
        if len(g) >= MIN_SLICE_COPIES:
            reads.append((g, [k for k in kernels if t0 <= k[0] < t1]))
    return reads


def landings(slice_copies, split=True):
    """When each slice had landed whole. split: every slice is copied half
    on either DMA stream and has landed when both halves have. The trace
    does not name the streams, so the copies are dealt to two lanes: a copy
    continues the lane that fell idle last before it started."""
    if not split:
        return sorted(c[1] for c in slice_copies)
    lanes = [[], []]
    for c in sorted(slice_copies):
        idle = [ln for ln in lanes if not ln or ln[-1][1] <= c[0] + 0.005]
        if idle:
            lane = max(idle, key=lambda ln: ln[-1][1] if ln else float("-inf"))
        else:
            lane = min(lanes, key=lambda ln: ln[-1][1])
        lane.append(c)
    n = min(len(lanes[0]), len(lanes[1]))
    out = [max(lanes[0][k][1], lanes[1][k][1]) for k in range(n)]
    out += [c[1] for ln in lanes for c in ln[n:]]
    return sorted(out)


def busy(spans):
    """Length of the union of (start, end) spans."""
    total, cur_s, cur_e = 0.0, None, None
    for s, e in sorted(spans):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                total += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        total += cur_e - cur_s
    return total


def report(idx, slice_copies, ks, detail, split):
    t0 = slice_copies[0][0]
    last_copy = max(c[1] for c in slice_copies)
    last_kernel = max((k[1] for k in ks), default=last_copy)
    after = [k for k in ks if k[1] > last_copy]
    print(f"read {idx}: {len(slice_copies)} slice copies, last lands at "
          f"{last_copy - t0:.3f} ms, last decode kernel ends at "
          f"{last_kernel - t0:.3f} ms: tail {last_kernel - last_copy:.3f} ms; "
          f"{len(after)} kernels end after the last copy, busy "
          f"{busy([(max(k[0], last_copy), k[1]) for k in after]):.3f} ms")
    if not detail:
        return
    print("  copies (start, end) ms from first issue:",
          [(round(c[0] - t0, 3), round(c[1] - t0, 3)) for c in slice_copies])
    print("  kernels (start, end, name) from first copy issue:")
    for s, e, name in ks:
        mark = " *" if e > last_copy else "  "
        print(f"  {mark}{s - t0:9.3f} {e - t0:8.3f}  {name[:72]}")
    print("  (* ends after the last copy)")
    counts = [i for i, k in enumerate(ks) if "frame_scan_pass_kernel<false>" in k[2]]
    land = landings(slice_copies, split)
    print("  slice: landed, period to the next landing, chain wall, chain busy")
    for n, i in enumerate(counts):
        j = counts[n + 1] if n + 1 < len(counts) else len(ks)
        chain = ks[i:j]
        wall = max(k[1] for k in chain) - chain[0][0]
        period = (f"{land[n + 1] - land[n]:.3f}" if n + 1 < len(land)
                  else "  -  ")
        landed = f"{land[n] - t0:.3f}" if n < len(land) else "  ?  "
        print(f"  {n:5d}  {landed:>7}  {period:>7}  {wall:7.3f}  "
              f"{busy([(k[0], k[1]) for k in chain]):7.3f}   "
              f"(COUNT starts {chain[0][0] - t0:.3f})")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out_dir")
    ap.add_argument("--read", type=int, default=-1,
                    help="read to print in detail (default: the last)")
    ap.add_argument("--whole-slices", action="store_true",
                    help="the run had TFREC_READ_SPLIT=0: one copy per slice")
    args = ap.parse_args()
    kernels, copies = load(args.out_dir)
    dirs = {}
    for c in copies:
        dirs[c[2]] = dirs.get(c[2], 0) + 1
    print("copy directions:", dirs)
    reads = find_reads(kernels, copies)
    if not reads:
        raise SystemExit("no slice copies found in the trace")
    detail = args.read % len(reads)
    for i, (g, ks) in enumerate(reads):
        report(i, g, ks, i == detail, not args.whole_slices)


if __name__ == "__main__":
    main()
