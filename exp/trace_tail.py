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
the slice period (the distance between two landings). Per read it also
prints the link's busy share between the first and the last slice copy, the
largest idle gap between copies, and how long the device had been idle of
this process's work when the first slice copy started (the end of the write
before it, then the read's host-side head; an upper bound of that head).
--min-copy-ms lowers the slice-copy threshold for reads whose slices are
copied in small chunks (the per-slice landing table then no longer applies).

--writes prints the write side instead. A write starts at its first kernel
(size_records) and ends where the next read's first slice copy is issued.
Per write: the head (first kernel's start to the start of the first large
device-to-host copy), the end (last large copy's end to the end of the
call's last device activity) and what lies in each.
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


def find_writes(kernels, copies):
    """[(t0, t1, large D2H copies, kernels, small copies)] per write."""
    starts = [k[0] for k in kernels if "size_records" in k[2]]
    reads = [c[0] for c in copies if "HOST_TO_DEVICE" in c[2]
             and c[1] - c[0] > SLICE_COPY_MS]
    writes = []
    for i, t0 in enumerate(starts):
        t1 = min([r for r in reads if r > t0] + starts[i + 1:i + 2] +
                 [float("inf")])
        inside = [c for c in copies if t0 <= c[0] < t1]
        big = [c for c in inside if "DEVICE_TO_HOST" in c[2]
               and c[1] - c[0] > SLICE_COPY_MS]
        ks = [k for k in kernels if t0 <= k[0] < t1]
        # a copy into pinned (not registered) memory can run as a blit
        # kernel, which the copy trace does not list
        blits = [k for k in ks if "copyBuffer" in k[2]
                 and k[1] - k[0] > SLICE_COPY_MS]
        big += [(k[0], k[1], "blit") for k in blits]
        if big:
            writes.append((t0, t1, big, [k for k in ks if k not in blits],
                           [c for c in inside if c not in big]))
    return writes


def report_write(idx, w, detail):
    t0, _, big, ks, small = w
    first, last = min(c[0] for c in big), max(c[1] for c in big)
    acts = [(k[0], k[1], k[2]) for k in ks] + \
           [(c[0], c[1], "copy " + c[2]) for c in small]
    end = max([a[1] for a in acts] + [last])
    link = busy([(c[0], c[1]) for c in big])
    print(f"write {idx}: {len(big)} slice copies, head {first - t0:.3f} ms, "
          f"copies {last - first:.3f} ms (link busy {link:.3f}), end "
          f"{end - last:.3f} ms, device span {end - t0:.3f} ms, last "
          f"device activity starts {max(a[0] for a in acts) - last:.3f} ms "
          f"after the last copy")
    if not detail:
        return
    print("  in the head (start, end, what) ms from the first kernel:")
    for s, e, name in sorted(a for a in acts if a[0] < first):
        print(f"    {s - t0:8.3f} {e - t0:8.3f}  {name[:72]}")
    print("  after the last copy:")
    for s, e, name in sorted(a for a in acts if a[1] > last):
        print(f"    {s - t0:8.3f} {e - t0:8.3f}  {name[:72]}")
    print("  slice copies (start, end):",
          [(round(c[0] - t0, 3), round(c[1] - t0, 3)) for c in sorted(big)])
    print("  emit kernels (start, end):",
          [(round(k[0] - t0, 3), round(k[1] - t0, 3)) for k in ks
           if "emit_records" in k[2]])


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


def report(idx, slice_copies, ks, detail, split, before=None):
    t0 = slice_copies[0][0]
    last_copy = max(c[1] for c in slice_copies)
    spans = sorted((c[0], c[1]) for c in slice_copies)
    link = busy(spans)
    gaps, end = [], spans[0][1]
    for s, e in spans[1:]:
        gaps.append(max(0.0, s - end))
        end = max(end, e)
    idle = f"{t0 - before:.3f}" if before is not None else "?"
    print(f"read {idx}: link busy {link:.3f} of {last_copy - t0:.3f} ms "
          f"({100 * link / (last_copy - t0):.0f}%), largest idle gap "
          f"{max(gaps, default=0.0):.3f} ms, idle gaps over 0.05 ms sum "
          f"{sum(g for g in gaps if g > 0.05):.3f} ms; first copy starts "
          f"{idle} ms after the device's last activity before it")
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
    global SLICE_COPY_MS
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out_dir")
    ap.add_argument("--read", type=int, default=-1,
                    help="read to print in detail (default: the last)")
    ap.add_argument("--whole-slices", action="store_true",
                    help="the run had TFREC_READ_SPLIT=0: one copy per slice")
    ap.add_argument("--min-copy-ms", type=float, default=SLICE_COPY_MS,
                    help="a copy longer than this is a slice (chunk) copy")
    ap.add_argument("--writes", action="store_true",
                    help="report the writes' head and end instead")
    args = ap.parse_args()
    SLICE_COPY_MS = args.min_copy_ms
    kernels, copies = load(args.out_dir)
    dirs = {}
    for c in copies:
        dirs[c[2]] = dirs.get(c[2], 0) + 1
    print("copy directions:", dirs)
    if args.writes:
        writes = find_writes(kernels, copies)
        if not writes:
            raise SystemExit("no sliced write found in the trace")
        for i, w in enumerate(writes):
            report_write(i, w, i == args.read % len(writes))
        return
    reads = find_reads(kernels, copies)
    if not reads:
        raise SystemExit("no slice copies found in the trace")
    detail = args.read % len(reads)
    ends = sorted([k[1] for k in kernels] + [c[1] for c in copies])
    for i, (g, ks) in enumerate(reads):
        before = max((e for e in ends if e <= g[0][0]), default=None)
        report(i, g, ks, i == detail, not args.whole_slices, before)


if __name__ == "__main__":
    main()
