#!/usr/bin/env python3
"""Time of the index query (ugpu_index_query) over the index
tables of the three shapes of tools/bench_index.py (the same text: 1 GiB as one
input, 4096 inputs of 256 KiB, 65536 inputs of 1 KiB, accuracy 4) and of two
more whose tables have 2 and 4 KiB (16384 inputs of 4 KiB, 8192 of 8 KiB), for
three patterns: a literal, a set of 100 words and [a-z]+(ing|ed).

The inputs are indexed on the device once (ugpu_index_tables); the query then
runs over the tables resident in HBM.  Per shape and pattern, medians of
--steps calls after --warmup of two clocks: ms_device*, the device time of the
kernel between two hipEvents (ugpu_index_query_kernel_ms), and ms_query / ms_lds*
/ ms_force_lds, a host clock around the synchronous call (the records' headers
and offsets to the device, the kernel, the keep bytes back).
  ms_query         the default switch (tables of up to ugpu_index_query_lds()
                   bytes are staged in LDS, larger ones probed in global memory)
  ms_lds_<N>       the same with the switch at N bytes (UGPU_QUERY_LDS_BYTES;
                   0 = every table probed in global memory)
  ms_force_lds     every table staged (UGPU_QUERY_FORCE_LDS: 64 KiB of LDS per
                   wave, two waves to a workgroup)
kept is the number of records the query keeps, the same under every setting
(asserted) and equal to the host evaluator's on a sample.

--cli UGREP adds, as context and not as a bar, the wall time of the reference
CLI `ugrep --index=fast -rl` (and plain `-rl`) over the same bytes as files in
a temporary directory with the store ugpu_index_batch's records give.

Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

# the three shapes of tools/bench_index.py, and two whose tables (2 and 4 KiB) lie at the switch
SHAPES = [("65536x1KiB", 65536, 1 << 10), ("16384x4KiB", 16384, 4 << 10), ("8192x8KiB", 8192, 8 << 10),
          ("4096x256KiB", 4096, 256 << 10), ("1x1GiB", 1, 1 << 30)]
SWITCHES = (0, 1024, 2048, 4096)


def timed(fn, warmup, steps, device_ms):
    """Medians of the call's host time and of its device time (device_ms() after each call), and the host min and max."""
    for _ in range(warmup):
        fn()
    ts, ds = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        ds.append(device_ms())
    ts.sort()
    ds.sort()
    return round(ts[len(ts) // 2], 4), round(ds[len(ds) // 2], 4), round(ts[0], 4), round(ts[-1], 4)


def shape_bytes(pool, count, size):
    """index_model.bench_input(pool, i, size) for i in 0..count-1, back to back, as one array."""
    import numpy as np
    n = pool.size
    out = np.empty(count * size, np.uint8)
    for i in range(count):
        start = (i * 7919 * 64) % n
        done = 0
        while done < size:
            c = min(size - done, n - start)
            out[i * size + done:i * size + done + c] = pool[start:start + c]
            done += c
            start = 0
    return out


def cli_times(ugrep, U, host, count, size, patterns):
    import numpy as np
    inputs = [host[i * size:(i + 1) * size] for i in range(count)]
    res = U.index_batch(inputs)
    names = ["f%05d.txt" % i for i in range(count)]
    out = {}
    with tempfile.TemporaryDirectory() as d:
        old = time.time() - 1000
        for nm, data in zip(names, inputs):
            with open(os.path.join(d, nm), "wb") as f:
                f.write(np.asarray(data).tobytes())
            os.utime(os.path.join(d, nm), (old, old))
        with open(os.path.join(d, "._UG#_Store"), "wb") as f:
            f.write(U.write_index_store(names, res))
        for label, pat in patterns:
            row = {}
            for key, args in (("s_index_fast", ["--index=fast", "-rl"]), ("s_plain", ["-rl"])):
                best, files = None, 0
                for _ in range(2):
                    t0 = time.perf_counter()
                    r = subprocess.run([ugrep] + args + ["-e", pat, "."], cwd=d, stdin=subprocess.DEVNULL,
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                    dt = time.perf_counter() - t0
                    assert r.returncode in (0, 1), r.stderr[-300:]
                    files = len(r.stdout.split())
                    best = dt if best is None else min(best, dt)
                row[key] = round(best, 4)
                row["files_listed"] = files
            out[label] = row
    return out


def run(args):
    import numpy as np
    import torch

    import hfa_model as H
    import index_model as M
    import ugrep_amd as U
    from ugrep_amd import _lib
    assert torch.cuda.is_available(), "bench_index_query needs a GPU"
    torch.cuda.set_device(0)
    patterns = [("literal", "kernel of the"), ("words100", "|".join(H.word_set())), ("loop_suffix", "[a-z]+(ing|ed)")]
    queries = [(label, pat, U.IndexQuery(pat)) for label, pat in patterns]
    pool = np.frombuffer(M.bench_pool(), np.uint8)
    out = dict(what="index query on one MI355X over the tables of the file index (accuracy 4) resident in HBM: "
                    "ms_device* = the kernel between two hipEvents, the others = a host clock around the synchronous "
                    "call; medians of --steps calls (ms)",
               steps=args.steps, warmup=args.warmup, default_switch_bytes=int(U.lib.ugpu_index_query_lds()),
               patterns={label: dict(pattern=pat if len(pat) < 60 else pat[:57] + "...", **q.info)
                         for label, pat, q in queries}, shapes={})
    for label, count, size in SHAPES:
        if args.shapes and label not in args.shapes:
            continue
        count = max(1, count // args.shrink)
        host = shape_bytes(pool, count, size)
        n = host.size
        bounds = np.arange(count + 1, dtype=np.uint64) * np.uint64(size)
        buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        buf[:n] = torch.from_numpy(host)
        torch.cuda.synchronize()
        header, _, offset, total = U.index_tables(buf.data_ptr(), n, bounds)
        dst = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        header, _, offset, total = U.index_tables(buf.data_ptr(), n, bounds, d_tables=dst.data_ptr(), capacity=total)
        del buf
        tabs = dst[:total].cpu().numpy()
        sizes = np.diff(offset.astype(np.int64))
        shape = dict(records=count, input_bytes=size, tables_bytes=int(total),
                     table_sizes={str(int(s)): int((sizes == s).sum()) for s in np.unique(sizes)}, patterns={})
        form = (dst.data_ptr(), header, offset)
        for plabel, _, q in queries:
            keep = q.query(form)
            row = dict(kept=int(keep.sum()))
            sample = list(range(0, count, max(1, count // 64)))
            row["host_agrees"] = all(
                bool(keep[i]) == q.keep_host(int(header[i]), tabs[int(offset[i]):int(offset[i + 1])]) for i in sample)
            dms = U.IndexQuery.kernel_ms
            row["ms_query"], row["ms_device"], row["ms_query_min"], row["ms_query_max"] = timed(
                lambda: q.query(form), args.warmup, args.steps, dms)
            for sw in SWITCHES:
                os.environ["UGPU_QUERY_LDS_BYTES"] = str(sw)
                assert np.array_equal(q.query(form), keep)
                row["ms_lds_%d" % sw], row["ms_device_lds_%d" % sw] = timed(lambda: q.query(form), args.warmup, args.steps, dms)[:2]
            del os.environ["UGPU_QUERY_LDS_BYTES"]
            assert np.array_equal(q.query(form, force="lds"), keep)
            row["ms_force_lds"], row["ms_device_force_lds"] = timed(lambda: q.query(form, force="lds"), args.warmup,
                                                                    args.steps, dms)[:2]
            shape["patterns"][plabel] = row
        del dst
        torch.cuda.empty_cache()
        out["shapes"][label] = shape
        write(args, out)  # (after every step: a long run leaves what it has)
        if args.cli:
            shape["reference_cli"] = cli_times(os.path.abspath(args.cli), U, host, count, size, patterns)
            write(args, out)
    if args.cli:
        out["reference_cli"] = ("context, not a bar: wall seconds of the reference ugrep --index=fast -rl and ugrep -rl "
                                "over the same bytes as files (page cache warm, best of 2), whose time is reading and "
                                "searching the kept files; ms_query above is the query over the tables alone")
    out["library"] = _lib.build_id()[0]
    return out


def write(args, doc):
    # (innermost objects on one line)
    text = re.sub(r"\{\n\s+([^{}]*?)\n\s*\}", lambda m: "{" + re.sub(r"\n\s+", " ", m.group(1)) + "}", json.dumps(doc, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="*", default=[], help="a subset of: " + " ".join(s[0] for s in SHAPES))
    ap.add_argument("--shrink", type=int, default=1, help="divide every shape's input count (rehearsals)")
    ap.add_argument("--cli", default="", metavar="UGREP", help="also time the reference CLI (context)")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    args = ap.parse_args()
    doc = run(args)
    write(args, doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
