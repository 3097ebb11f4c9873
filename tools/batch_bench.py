#!/usr/bin/env python3
"""Batched FIND against the per-input loop it replaces.

For each pattern (C2 foo|bar|baz over the word corpus, C3 identifiers over the
code corpus) and each shape (inputs x bytes), the same host inputs go through
  batch: one ugpu_find_batch call, and
  loop:  one ugpu_find_all call per input (how a caller did this work before
         ugpu_find_batch existed),
both at the C ABI (no Python conversion inside the timed region), OFFSETS
mode, warm pools, wall time from the call to the return (both calls are
synchronous) followed by a device synchronise; the median of --runs runs.  The
totals of the two are compared.  Alongside, ugpu_split_matches is timed alone
on the packed buffer and the packed scan's device match list, with its share
of the batch time, and the batch in COUNT mode (batch_count_ms: the same device
work without the record copy to the host).  Prints one JSON line per case and
writes all of them to --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import ugrep_amd  # noqa: E402
from ugrep_amd import _lib  # noqa: E402

PATTERNS = {"c2": ("c2_foobarbaz", ugrep_amd.GEN_WORDS), "c3": ("c3_ident", ugrep_amd.GEN_CODE)}
SHAPES = "65536x1024,4096x16384,256x1048576"


def corpus(kind, n):
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    ugrep_amd.gen(kind, 1, 0, buf.data_ptr(), n)
    torch.cuda.synchronize()
    return buf[:n].cpu().numpy()


def timed(f, runs):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), r


def split_alone(pat, inputs, runs):
    """ugpu_split_matches alone over the packed inputs and their device list."""
    parts, bounds, off = [], [], 0
    for d in inputs:
        bounds.append(off)
        parts.append(d)
        off += d.size
        if d.size and d[-1] != 10:
            parts.append(np.array([10], np.uint8))
            off += 1
    bounds.append(off)
    packed = np.concatenate(parts)
    nseg = len(inputs)
    dbuf = torch.zeros(off + 16, dtype=torch.uint8, device="cuda")
    dbuf[:off].copy_(torch.from_numpy(packed))
    db = torch.from_numpy(np.asarray(bounds, np.uint64).view(np.int64)).to("cuda")
    sc = ugrep_amd.Scanner(pat, records=True)
    sc.scan(dbuf.data_ptr(), 0, off, off, True, 0, 0)
    n = sc.totals().count
    st = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    ln = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    cp = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    sc.offsets(st.data_ptr(), ln.data_ptr(), cp.data_ptr(), n, 0)
    seg = torch.empty((5, nseg + 1), dtype=torch.int64, device="cuda")
    rec = torch.empty((2, max(n, 1)), dtype=torch.int64, device="cuda")

    def run():
        ugrep_amd.split_matches(dbuf.data_ptr(), off, db.data_ptr(), nseg, st.data_ptr(), ln.data_ptr(),
                                cp.data_ptr(), 0, n, seg[0].data_ptr(), seg[1].data_ptr(), seg[2].data_ptr(),
                                seg[3].data_ptr(), seg[4].data_ptr(), rec[0].data_ptr(), rec[1].data_ptr())

    run()
    med, best, _ = timed(run, runs)
    sc.close()
    return med, best, n, off


def case(name, pat, host, count, size, runs):
    inputs = [host[i * size:(i + 1) * size] for i in range(count)]
    ptrs = (ctypes.c_void_p * count)(*[d.ctypes.data for d in inputs])
    lens = (ctypes.c_uint64 * count)(*[d.size for d in inputs])
    h = pat.handle

    def batch(mode=_lib.MODE_OFFSETS):
        res = ctypes.POINTER(_lib.BatchResult)()
        _lib.check(_lib.lib.ugpu_find_batch(h, ptrs, lens, count, mode, ctypes.byref(res)))
        r = res.contents
        tot = (r.count, int(np.ctypeslib.as_array(r.digest, shape=(count,)).sum(dtype=np.uint64)), bool(r.flags & 1))
        _lib.lib.ugpu_batch_free(res)
        return tot

    def loop():
        cnt = dg = 0
        res = ctypes.POINTER(_lib.Result)()
        find_all, free = _lib.lib.ugpu_find_all, _lib.lib.ugpu_result_free
        for i in range(count):
            rc = find_all(h, ptrs[i], size, 0, _lib.MODE_OFFSETS, ctypes.byref(res))
            if rc:
                _lib.check(rc)
            cnt += res.contents.count
            dg += res.contents.digest
            free(res)
        return cnt, dg & 0xFFFFFFFFFFFFFFFF

    batch()  # warm pools
    b_med, b_min, btot = timed(batch, runs)
    # COUNT mode: the same device work without the record copy to the host
    c_med, c_min, ctot = timed(lambda: batch(_lib.MODE_COUNT), runs)
    loop()
    l_med, l_min, ltot = timed(loop, runs)
    assert btot[:2] == ltot and ctot == btot, (btot, ctot, ltot)
    s_med, s_min, n, packed = split_alone(pat, inputs, runs)
    return {"pattern": name, "inputs": count, "input_bytes": size, "packed_bytes": packed, "matches": btot[0],
            "one_scan": btot[2], "runs": runs, "batch_ms": round(b_med, 3), "batch_min_ms": round(b_min, 3),
            "batch_count_ms": round(c_med, 3),
            "loop_ms": round(l_med, 3), "loop_min_ms": round(l_min, 3), "loop_over_batch": round(l_med / b_med, 2),
            "split_ms": round(s_med, 3), "split_min_ms": round(s_min, 3), "split_share": round(s_med / b_med, 4),
            "batch_GBps": round(count * size / b_med / 1e6, 3), "loop_GBps": round(count * size / l_med / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="c2,c3")
    ap.add_argument("--shapes", default=SHAPES, help="inputs x bytes, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(REPO, "ugrep_amd", "data", "config_patterns.json")) as f:
        cfg = json.load(f)
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    need = max(c * s for c, s in shapes)
    rows = []
    for name in args.patterns.split(","):
        key, kind = PATTERNS[name]
        pat = ugrep_amd.Pattern(cfg[key]["opc"])
        host = corpus(kind, need)
        for count, size in shapes:
            row = case(name, pat, host, count, size, args.runs)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump({"device": torch.cuda.get_device_name(0), "build": ugrep_amd._lib.build_id()[0],
                               "mode": "OFFSETS", "timing": "wall ms, median of runs, device synchronised",
                               "cases": rows}, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
