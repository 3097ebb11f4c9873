#!/usr/bin/env python3
"""Two-field against three-field prefilter (DESIGN 3.1, tables.hpp
kFilter2Added): scan-kernel time of foo|bar|baz over 1 GiB of the C2 corpus
with alias trigrams (`&//`, `"!2`, `"!:`: candidates of the two-field form
only) planted at rising densities, under UGPU_FT2=0 and UGPU_FT2=1.  One JSON
line per density, then a summary line; --out also writes the summary to a
file.  The density at which the two-field kernel stops being faster, halved,
is the bound kFilter2Added."""
import argparse
import json
import os
import sys

import torch

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [_ROOT]
import ugrep_amd as U  # noqa: E402

TRIGRAMS = (b"&//", b'"!2', b'"!:')


def kernel_ms(pat, buf, n, ft2, steps, warmup):
    """(median kernel ms, fastest, match count) of COUNT scans under UGPU_FT2=ft2."""
    st = torch.cuda.current_stream().cuda_stream
    os.environ["UGPU_FT2"] = str(ft2)
    try:
        sc = U.Scanner(pat)
        ms = []
        for i in range(warmup + steps):
            sc.scan(buf.data_ptr(), 0, n, n, True, 0, st)
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append(sc.kernel_ms())
        cnt = sc.totals().count
        sc.close()
    finally:
        os.environ.pop("UGPU_FT2", None)
    ms.sort()
    return ms[len(ms) // 2], ms[0], cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--densities", default="0,1e-6,1e-5,1e-4,1e-3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.mib << 20
    torch.cuda.set_device(0)
    pat = U.Pattern("foo|bar|baz")
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    tri = torch.tensor([list(t) for t in TRIGRAMS], dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda")
    rows = []
    for d in (float(x) for x in args.densities.split(",")):
        U.gen(U.GEN_WORDS, 1, 0, buf.data_ptr(), n)
        k = int(d * n)
        if k:
            g.manual_seed(7)
            pos = torch.randint(0, n - 3, (k,), generator=g, device="cuda")
            which = tri[pos % 3]
            for j in range(3):
                buf[pos + j] = which[:, j]
        torch.cuda.synchronize()
        row = {"alias_trigrams_per_byte": d, "planted": k, "bytes": n}
        for ft2 in (0, 1):
            med, best, cnt = kernel_ms(pat, buf, n, ft2, args.steps, args.warmup)
            row["ft2_%d" % ft2] = {"kernel_ms": round(med, 4), "kernel_ms_min": round(best, 4), "count": cnt}
        assert row["ft2_0"]["count"] == row["ft2_1"]["count"], row
        row["ft2_1_over_ft2_0"] = round(row["ft2_1"]["kernel_ms"] / row["ft2_0"]["kernel_ms"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    faster = [r["alias_trigrams_per_byte"] for r in rows if r["ft2_1_over_ft2_0"] < 1.0]
    out = {"what": "sparse_kernel foo|bar|baz, %d MiB kind-1 corpus, alias trigrams planted; kernel_ms = median of %d"
                   % (args.mib, args.steps),
           "device": torch.cuda.get_device_name(0), "rows": rows,
           "largest_density_still_faster": max(faster) if faster else None}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
