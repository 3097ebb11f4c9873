#!/usr/bin/env python3
"""Throughput of the file index (ugpu_index_tables / ugpu_index_batch, DESIGN
§3.5.5) on three shapes of the same text (tests/index_model.py bench_pool):
1 GiB as one input, 4096 inputs of 256 KiB and 65536 inputs of 1 KiB, at
accuracy 4.

Per shape, each timed on its own with a host clock around the synchronous call
(median of --steps calls after --warmup):
  ms_device_query  ugpu_index_tables as a size query over the inputs resident
                   in HBM: flags, hash, fold, and the per-input results to the
                   host
  ms_device_call   the same with the tables written compactly to a device buffer
  ms_batch         ugpu_index_batch from host memory: packing through pinned
                   memory, the copy to the device, the call, the tables back to
                   the host (end to end)
Kernel times come from a separate run of the same command under
  rocprofv3 --kernel-trace --output-format csv
(tracing slows the host, so that run's call times are not used); --merge-trace
CSV adds, per shape, the mean duration of each kernel over the timed
ms_device_call calls to the JSON in --out: the dispatches of a kernel are
given to the shapes and calls in the order they ran.  From the hash kernel's
time: the input rate, its share of the 8 TB/s of HBM, and the LDS atomics
(eight per input byte) per second and per CU and clock (256 CUs, 2.4 GHz).

--baseline FILE merges the reference indexer's seconds on the same bytes
(tests/golden/make_index_golden.py --time, one CPU thread) and the ratios.

Prints one JSON object; --out also writes it to a file."""
import argparse
import csv
import json
import os
import re
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ROOFLINE = 8.0e12
CUS, CLOCK = 256, 2.4e9
SHAPES = [("1x1GiB", 1, 1 << 30), ("4096x256KiB", 4096, 256 << 10), ("65536x1KiB", 65536, 1 << 10)]
KERNELS = ("idx_flag_kernel", "idx_hash_kernel", "idx_fold_kernel", "idx_emit_kernel")


def timed(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def run(args):
    import numpy as np
    import torch

    import index_model as M
    import ugrep_amd as U
    from ugrep_amd import _lib
    assert torch.cuda.is_available(), "bench_index needs a GPU"
    torch.cuda.set_device(0)
    pool = M.bench_pool()
    chunk = U.index_chunk()
    out = dict(what="file index on one MI355X, accuracy 4: size query and whole call over inputs in HBM, and "
                    "ugpu_index_batch from host memory; median of --steps calls (ms)",
               roofline_GBps=ROOFLINE / 1e9, steps=args.steps, warmup=args.warmup, chunk=chunk, shapes={})
    w, s = args.warmup, args.steps
    for label, count, size in SHAPES:
        if args.shapes and label not in args.shapes:
            continue
        count = max(1, count // args.shrink)
        inputs = [np.frombuffer(M.bench_input(pool, i, size), np.uint8) for i in range(count)]
        n = count * size
        bounds = np.arange(count + 1, dtype=np.uint64) * np.uint64(size)
        buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        buf[:n] = torch.from_numpy(np.concatenate(inputs) if count > 1 else inputs[0].copy())
        torch.cuda.synchronize()
        header, zeros, offset, total = U.index_tables(buf.data_ptr(), n, bounds)
        dst = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        q = timed(lambda: U.index_tables(buf.data_ptr(), n, bounds), w, s)
        c = timed(lambda: U.index_tables(buf.data_ptr(), n, bounds, d_tables=dst.data_ptr(), capacity=total), w, s)
        res = [None]

        def batch():
            res[0] = U.index_batch(inputs)
        b = timed(batch, w, s)
        # the records of the first input (and of the last, when small) are the model's; batch and device call agree
        tabs = dst[:total].cpu().numpy()
        ok = bool(np.array_equal(res[0].tables, tabs) and np.array_equal(res[0].header, header))
        for i in ([0] if size > (1 << 20) else [0, count - 1]):
            if size <= (4 << 20) or args.check_large:
                h, t, z = M.index_record(inputs[i])
                ok = ok and (int(header[i]), int(zeros[i])) == (h, z) and res[0].table(i) == t
        multi = 1 if size > chunk else 0
        calls = 1 + 2 * (w + s) + (w + s)
        out["shapes"][label] = dict(
            inputs=count, input_bytes=size, bytes=n, tables_bytes=int(total), records_ok=ok,
            ms_device_query=round(q[0], 4), ms_device_query_min=round(q[1], 4),
            ms_device_call=round(c[0], 4), ms_device_call_min=round(c[1], 4), ms_device_call_max=round(c[2], 4),
            ms_batch=round(b[0], 3), ms_batch_min=round(b[1], 3), ms_batch_max=round(b[2], 3),
            GBps_device_call=round(n / c[0] / 1e6, 2), GBps_batch=round(n / b[0] / 1e6, 3),
            dispatches=dict(idx_flag_kernel=calls, idx_hash_kernel=calls, idx_fold_kernel=calls * multi,
                            idx_emit_kernel=2 * (w + s)))
        del buf, dst, inputs
        torch.cuda.empty_cache()
    out["library"] = _lib.build_id()[0]
    return out


def merge_trace(doc, path):
    """Mean kernel durations per shape, over the timed ms_device_call calls,
    from a rocprofv3 kernel trace (CSV) of a run of this tool with the same
    shapes, warmup and steps."""
    w, s = doc["warmup"], doc["steps"]
    rows = {k: [] for k in KERNELS}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    used = {k: 0 for k in KERNELS}
    for label, c in doc["shapes"].items():
        c["kernels"] = {}
        for k in KERNELS:
            count = c["dispatches"][k]
            mine = sorted(rows[k])[used[k]:used[k] + count]
            assert len(mine) == count, (label, k, len(mine), count)
            used[k] += count
            if not count:
                continue
            # order of the calls: one size query, w + s queries, w + s whole calls, w + s batches (no emit in a query)
            first = w if k == "idx_emit_kernel" else 1 + (w + s) + w
            ns = [e - b for b, e in mine[first:first + s]]
            c["kernels"][k] = dict(calls=len(ns), mean_ns=round(sum(ns) / len(ns), 1), min_ns=min(ns), max_ns=max(ns))
        t = c["kernels"]["idx_hash_kernel"]["mean_ns"] * 1e-9
        c["hash_kernel"] = dict(GBps_input=round(c["bytes"] / t / 1e9, 1), share_of_hbm=round(c["bytes"] / t / ROOFLINE, 4),
                                lds_atomics_per_s=round(8 * c["bytes"] / t, 0),
                                lds_atomics_per_cu_clock=round(8 * c["bytes"] / t / CUS / CLOCK, 2))
        c["kernel_ns_per_call"] = round(sum(v["mean_ns"] for v in c["kernels"].values()), 1)
    doc["kernels_from"] = "a separate rocprofv3 --kernel-trace run of the same command (mean ns over the timed whole calls)"
    return doc


def merge_baseline(doc, path):
    with open(path) as f:
        base = json.load(f)
    doc["baseline"] = dict(what="the reference ugrep-indexer -4 on the same bytes as files, page cache warm, best of 2 "
                                "(tests/golden/make_index_golden.py --time), on the CPU of the build machine",
                           threads=1, shapes=base)
    for label, c in doc["shapes"].items():
        if label in base and base[label]["bytes"] == c["bytes"]:
            c["baseline_seconds"] = round(base[label]["seconds"], 3)
            c["baseline_over_batch"] = round(base[label]["seconds"] * 1e3 / c["ms_batch"], 1)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", nargs="*", default=[], help="a subset of: " + " ".join(s[0] for s in SHAPES))
    ap.add_argument("--shrink", type=int, default=1, help="divide every shape's input count (rehearsals)")
    ap.add_argument("--check-large", action="store_true", help="also compare a 1 GiB input's record with the model")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    ap.add_argument("--merge-trace", default="", metavar="CSV",
                    help="with --out: add the kernel times of this rocprofv3 kernel trace to the JSON in --out; no GPU run")
    ap.add_argument("--baseline", default="", metavar="JSON",
                    help="with --out: add the reference indexer's times to the JSON in --out; no GPU run")
    args = ap.parse_args()
    if args.merge_trace or args.baseline:
        with open(args.out) as f:
            doc = json.load(f)
        if args.merge_trace:
            doc = merge_trace(doc, args.merge_trace)
        if args.baseline:
            doc = merge_baseline(doc, args.baseline)
    else:
        doc = run(args)
    # (innermost objects on one line)
    text = re.sub(r"\{\n\s+([^{}]*?)\n\s*\}", lambda m: "{" + re.sub(r"\n\s+", " ", m.group(1)) + "}", json.dumps(doc, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
