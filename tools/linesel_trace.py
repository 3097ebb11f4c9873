#!/usr/bin/env python3
"""Per-pass kernel times of `tools/bench_lines.py --select` from a rocprofv3
kernel trace of that run:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- \\
        python3 tools/bench_lines.py --config c2 --select --steps 5 --warmup 1
    python3 tools/linesel_trace.py DIR --steps 5 --warmup 1

The select-count pass of the plain and of the inverted calls is the same
kernel (sel_kernel<false>); the bench issues its calls in a fixed order, so the
dispatches are told apart by position.  Prints one JSON object: average
milliseconds per dispatch of every pass.
"""
import argparse
import csv
import glob
import json
import os


def rows(d):
    out = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                r = {k.lower(): v for k, v in r.items()}
                out.append((int(r["start_timestamp"]), int(r["end_timestamp"]), r["kernel_name"]))
    out.sort()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    k = args.steps + args.warmup
    # the select-count dispatches in bench order: the sizing call, k x (write, count, inverted),
    # then the three timed loops
    order = ["plain"] + ["plain", "plain", "inverted"] * k + ["plain"] * (2 * k) + ["inverted"] * k
    acc = {}
    ncount = 0
    for t0, t1, name in rows(args.dir):
        if "sel_summary_kernel" in name:
            key = "summary"
        elif "sel_kernel<true>" in name:
            key = "select_write"
        elif "sel_kernel<false>" in name:
            key = "select_count_" + (order[ncount] if ncount < len(order) else "unordered")
            ncount += 1
        elif "nl_count_kernel" in name:
            key = "nl_count_kernel"
        elif "nl_assign" in name:
            key = "nl_assign_kernel"
        else:
            continue
        acc.setdefault(key, []).append((t1 - t0) / 1e6)
    out = {key: {"calls": len(v), "avg_ms": round(sum(v) / len(v), 4), "min_ms": round(min(v), 4)}
           for key, v in sorted(acc.items())}
    out["select_count_dispatches_as_expected"] = ncount == len(order)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
