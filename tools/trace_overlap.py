#!/usr/bin/env python3
"""usage: tools/trace_overlap.py <kernel_trace.csv> [--kernel REGEX] [--last N]
Reads a `rocprofv3 --kernel-trace --output-format csv` trace and reports, for the dispatches that carry the last N solves of the kernels
that match (the timed block of a bench.py run: everything before it is warm-up and the first replay), how far they overlap: the span from
the first start to the last end, per dispatch and per solve, the mean kernel duration, and how many kernels started before the kernel
dispatched in front of them had ended.  A launch of solve_twisted_group_kernel or solve_twisted_group8_kernel (a replay with
UAVQP_CAPTURE_FUSE > 1: csrc/uavqp_capture.h) carries one solve per row of its grid (Grid_Size_Y); every other dispatch is one solve."""
import argparse
import csv
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--kernel", default="solve_twisted(_group8?)?_kernel")
    ap.add_argument("--last", type=int, default=40, help="solves (not dispatches) to look at, counted from the end of the trace")
    a = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(a.trace)):
        if re.search(a.kernel, r["Kernel_Name"]):
            solves = max(1, int(r.get("Grid_Size_Y") or 1) // max(1, int(r.get("Workgroup_Size_Y") or 1))) if re.search("_group8?_kernel", r["Kernel_Name"]) else 1
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), solves))
    rows.sort()
    kept, solves = [], 0
    for row in reversed(rows):
        if solves >= a.last:
            break
        kept.append(row)
        solves += row[2]
    rows = kept[::-1]
    n = len(rows)
    if n == 0:
        print("no dispatch matches")
        return
    span = max(e for _, e, _ in rows) - rows[0][0]
    mean = sum(e - s for s, e, _ in rows) / n
    early = sum(1 for (_, e0, _), (s1, _, _) in zip(rows, rows[1:]) if s1 < e0)
    gaps = sorted(s1 - e0 for (_, e0, _), (s1, _, _) in zip(rows, rows[1:])) or [0]
    print(f"{n} dispatches of {solves} solves: span {span / 1e3:.2f} us = {span / 1e3 / n:.3f} us per kernel = {span / 1e3 / solves:.3f} us per solve; "
          f"mean duration {mean / 1e3:.3f} us; {early} of {n - 1} started before the one in front had ended; "
          f"median start-after-previous-end {gaps[len(gaps) // 2] / 1e3:+.3f} us")


if __name__ == "__main__":
    main()
