#!/usr/bin/env python3
"""usage: tools/trace_overlap.py <kernel_trace.csv> [--kernel REGEX] [--last N]
Reads a `rocprofv3 --kernel-trace --output-format csv` trace and reports, for the last N dispatches of the kernels that match (the timed
block of a bench.py run: everything before it is warm-up and the first replay), how far they overlap: the span from the first start to
the last end, the mean kernel duration, and how many kernels started before the kernel dispatched in front of them had ended."""
import argparse
import csv
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--kernel", default="solve_twisted_kernel")
    ap.add_argument("--last", type=int, default=40)
    a = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(a.trace)):
        if re.search(a.kernel, r["Kernel_Name"]):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    rows = rows[-a.last:]
    n = len(rows)
    if n == 0:
        print("no dispatch matches")
        return
    span = max(e for _, e in rows) - rows[0][0]
    mean = sum(e - s for s, e in rows) / n
    early = sum(1 for (_, e0), (s1, _) in zip(rows, rows[1:]) if s1 < e0)
    gaps = sorted(s1 - e0 for (_, e0), (s1, _) in zip(rows, rows[1:]))
    print(f"{n} dispatches: span {span / 1e3:.2f} us = {span / 1e3 / n:.3f} us per kernel; mean duration {mean / 1e3:.3f} us; "
          f"{early} of {n - 1} started before the one in front had ended; median start-after-previous-end {gaps[len(gaps) // 2] / 1e3:+.3f} us")


if __name__ == "__main__":
    main()
