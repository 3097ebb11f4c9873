#!/usr/bin/env python3
"""Throughput of ugpu_transcode over 1 GiB of input resident in
HBM, per encoding: lorem-like text (tests/golden/verify/lorem.utf8.txt in that
encoding, repeated), and for UTF-16 also a surrogate-dense input (30 % high,
30 % low surrogates).

Per case and step, each timed on its own with a host clock around the
synchronous call: the size query (the summary pass and the stitch), the whole
call (summary, stitch, write pass), and a device-to-device copy of
2 x source + output bytes -- the bytes the two-pass design moves (the source is
read twice, the output written once), so the copy's time is what that many
bytes cost at this machine's copy rate.  Reported: times, bytes, the ratio of
the call to that copy, and the traffic of the call (2 x source + output) over
its time as a share of the 8 TB/s roofline.

Kernel times come from a separate run under  rocprofv3 --kernel-trace
--output-format csv  (tracing slows the host, so the call times of that run are
not used); --merge-trace FILE adds the mean duration of tc_summary_kernel and
tc_write_kernel per case to the JSON of the untraced run: the dispatches of a
kernel are given to the cases in the order the cases ran.

Prints one JSON object; --out also writes it to a file.
"""
import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROOFLINE = 8.0e12
KERNEL_ENC = {"utf16be": 2, "utf16le": 3, "utf32be": 4, "utf32le": 5, "latin1": 6, "page": 7, "null_data": 8}
CASES = [("utf16le_text", "utf16le"), ("utf16le_surrogates", "utf16le"), ("utf16be_text", "utf16be"),
         ("utf32le_text", "utf32le"), ("utf32be_text", "utf32be"), ("latin1_text", "latin1"), ("page_text", "page"),
         ("null_data_text", "null_data")]


def sample(case, enc):
    """(host bytes to repeat, page or None)"""
    import numpy as np
    text = open(os.path.join(REPO, "tests", "golden", "verify", "lorem.utf8.txt"), "rb").read().decode()
    page = None
    if case.endswith("surrogates"):
        rng = np.random.default_rng(1)
        m = 8 << 20
        kind = rng.random(m)
        u = np.where(kind < 0.3, rng.integers(0xD800, 0xDC00, m),
                     np.where(kind < 0.6, rng.integers(0xDC00, 0xE000, m), rng.integers(0x20, 0x2000, m)))
        return u.astype("<u2").tobytes(), None
    if enc.startswith("utf16"):
        return text.encode("utf-16-le" if enc == "utf16le" else "utf-16-be"), None
    if enc.startswith("utf32"):
        return text.encode("utf-32-le" if enc == "utf32le" else "utf-32-be"), None
    if enc == "page":
        page = [ord(bytes([b]).decode("cp1252", "replace")) for b in range(256)]
        return text.encode("cp1252", "replace"), page
    return text.encode("latin-1", "replace"), None


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

    import ugrep_amd as U
    from ugrep_amd import _lib
    assert torch.cuda.is_available(), "bench_transcode needs a GPU"
    torch.cuda.set_device(0)
    out = dict(what="ugpu_transcode on one MI355X: size query, whole call and a device-to-device copy of "
                    "2 x source + output bytes, median of --steps calls (ms)", roofline_GBps=ROOFLINE / 1e9,
               bytes=args.bytes, steps=args.steps, warmup=args.warmup, cases={})
    for case, enc in CASES:
        if args.cases and case not in args.cases:
            continue
        host, page = sample(case, enc)
        unit = 4 if enc.startswith("utf32") else 2 if enc.startswith("utf16") else 1
        n = args.bytes // unit * unit
        piece = torch.from_numpy(np.frombuffer(host, np.uint8).copy()).cuda()
        src = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        reps = (n + piece.numel() - 1) // piece.numel()
        src[:n] = piece.repeat(reps)[:n]
        del piece
        e = KERNEL_ENC[enc]
        torch.cuda.synchronize()
        m = U.transcode(src.data_ptr(), n, e, 0, page)
        assert m <= U.transcode_bound(e, n)
        dst = torch.zeros(m + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        q = timed(lambda: U.transcode(src.data_ptr(), n, e, 0, page), args.warmup, args.steps)
        c = timed(lambda: U.transcode(src.data_ptr(), n, e, 0, page, dst.data_ptr(), m), args.warmup, args.steps)
        # the output is what Python's codec gives for the first bytes of the text cases
        ok = None
        if not case.endswith("surrogates") and enc not in ("null_data",):
            k = min(len(host), n) // unit * unit
            want = host[:k].decode({"utf16le": "utf-16-le", "utf16be": "utf-16-be", "utf32le": "utf-32-le",
                                    "utf32be": "utf-32-be", "latin1": "latin-1", "page": "cp1252"}[enc]).encode()
            ok = dst[:len(want)].cpu().numpy().tobytes() == want
        traffic = 2 * n + m
        a = torch.empty(traffic, dtype=torch.uint8, device="cuda")
        b = torch.empty(traffic, dtype=torch.uint8, device="cuda")
        a.fill_(1)
        cp = timed(lambda: b.copy_(a), args.warmup, args.steps)
        del a, b
        out["cases"][case] = dict(
            enc=enc, kernel_enc=e, source_bytes=n, output_bytes=m, output_ok=ok, traffic_bytes=traffic,
            ms_query=round(q[0], 4), ms_query_min=round(q[1], 4), ms_call=round(c[0], 4), ms_call_min=round(c[1], 4),
            ms_call_max=round(c[2], 4), ms_copy=round(cp[0], 4), ms_copy_min=round(cp[1], 4),
            call_over_copy=round(c[0] / cp[0], 3), GBps_source_call=round(n / c[0] / 1e6, 1),
            GBps_traffic_call=round(traffic / c[0] / 1e6, 1), share_of_roofline_call=round(traffic / (c[0] * 1e-3) / ROOFLINE, 3),
            GBps_copy_bytes=round(traffic / cp[0] / 1e6, 1),
            dispatches=dict(summary=1 + 2 * (args.warmup + args.steps), write=args.warmup + args.steps))
        del src, dst
        torch.cuda.empty_cache()
    out["library"] = _lib.build_id()[0]
    return out


def merge_trace(doc, path, warmup):
    """Mean kernel durations per case from a rocprofv3 kernel trace (CSV) of a
    run of this tool with the same cases, warmup and steps."""
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for v in rows.values():
        v.sort()
    used = {}
    for case, c in doc["cases"].items():
        for kind, count in c["dispatches"].items():
            names = [k for k in rows if "tc_%s_kernel<%d" % (kind, c["kernel_enc"]) in k]
            assert len(names) == 1, (kind, c["kernel_enc"], sorted(rows))
            at = used.get(names[0], 0)
            mine = rows[names[0]][at:at + count]
            assert len(mine) == count, (case, kind, len(mine), count)
            used[names[0]] = at + count
            skip = (1 + 2 * warmup) if kind == "summary" else warmup     # the first size query and the warm-up calls
            ns = [e - s for s, e in mine[skip:]]
            mean = sum(ns) / len(ns)
            nbytes = c["source_bytes"] + (c["output_bytes"] if kind == "write" else 0)
            c["kernel_" + kind] = dict(calls=len(ns), mean_ns=round(mean, 1), min_ns=min(ns), max_ns=max(ns), bytes=nbytes,
                                       GBps=round(nbytes / mean, 1), share_of_roofline=round(nbytes / (mean * 1e-9) / ROOFLINE, 3))
    doc["kernels_from"] = "a separate rocprofv3 --kernel-trace run of the same command (mean ns after the warm-up calls)"
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", nargs="*", default=[], help="a subset of: " + " ".join(c for c, _ in CASES))
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    ap.add_argument("--merge-trace", default="", metavar="CSV",
                    help="with --out: add the kernel times of this rocprofv3 kernel trace to the JSON in --out; no GPU run")
    args = ap.parse_args()
    if args.merge_trace:
        with open(args.out) as f:
            doc = json.load(f)
        doc = merge_trace(doc, args.merge_trace, doc["warmup"])
    else:
        doc = run(args)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
