#!/usr/bin/env python3
"""Throughput of the line-level consumers (ugpu_lines)
over a config's synthetic corpus resident in HBM.

The match starts come from one FIND scan (ugpu_scan + ugpu_scan_offsets) into
device arrays, as a line-mode ugrep consumer would get them; then each timed
step is one ugpu_lines call (newline count pass, host prefix of the per-wave
counts, line assignment pass, -c stitch).  Algorithmic bytes: the buffer is
read once plus 16 B per match (start read, line
written).  Prints one JSON line.  Profile with rocprofv3 --kernel-trace --stats
for the nl_count_kernel / nl_assign_kernel durations.

--select times the line records instead (ugpu_select_lines): per
step one call that writes the records of the matching lines (newline count,
summary, select-count and select-write passes), one count-only call and one
inverted count-only call, in that order, so a kernel trace of the run gives
the time of every pass (the select-count dispatches alternate plain, plain,
inverted) beside nl_count_kernel's.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import ugrep_amd  # noqa: E402

CONFIGS = {"c2": ("c2_foobarbaz", 1, 16 << 30), "c3": ("c3_ident", 3, 4 << 30), "c4": ("c4_word", 4, 4 << 30)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--bytes", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--select", action="store_true", help="time ugpu_select_lines instead of ugpu_lines")
    args = ap.parse_args()
    pkey, kind, size = CONFIGS[args.config]
    n = args.bytes or size
    with open(os.path.join(REPO, "ugrep_amd", "data", "config_patterns.json")) as f:
        opc = json.load(f)[pkey]["opc"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sptr = torch.cuda.current_stream(dev).cuda_stream
    buf = torch.empty(n + 16, dtype=torch.uint8, device=dev)
    ugrep_amd.gen(kind, 1, 0, buf.data_ptr(), n, sptr)
    pat = ugrep_amd.Pattern(opc)
    sc = ugrep_amd.Scanner(pat)
    sc.scan(buf.data_ptr(), 0, n, n, True, 0, sptr)
    t = sc.totals()
    m = t.count
    starts = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    lens = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    caps = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    sc.offsets(starts.data_ptr(), lens.data_ptr(), caps.data_ptr(), m, sptr)
    del caps
    if args.select:
        return select(args, dev, sptr, buf, n, starts, lens, m)
    del lens
    lines = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    for _ in range(args.warmup):
        nl, ml = ugrep_amd.lines(buf.data_ptr(), n, starts.data_ptr(), m, lines.data_ptr(), sptr)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        nl, ml = ugrep_amd.lines(buf.data_ptr(), n, starts.data_ptr(), m, lines.data_ptr(), sptr)
    torch.cuda.synchronize(dev)
    el = (time.perf_counter() - t0) / args.steps
    # sanity (not timed): newline count against torch, line numbers non-decreasing
    nl_torch = int((buf[:n] == 10).sum().item())
    mono = bool((lines[1:m] >= lines[:m - 1]).all().item()) if m > 1 else True
    alg = n + 16 * m  # every byte read once + start read + line written per match
    print(json.dumps({
        "what": "ugpu_lines (newline count + match line numbers + matching-line count)",
        "config": args.config, "bytes": n, "matches": m, "newlines": nl, "matching_lines": ml,
        "newlines_ok": nl == nl_torch, "lines_monotone": mono,
        "ms_per_call": round(el * 1e3, 4), "GBps_input": round(n / el / 1e9, 1),
        "GBps_algorithmic": round(alg / el / 1e9, 1), "algorithmic_bytes": alg}), flush=True)


def select(args, dev, sptr, buf, n, starts, lens, m):
    def timed(fn):
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize(dev)
        return out, (time.perf_counter() - t0) / args.steps

    bp, sp, lp = buf.data_ptr(), starts.data_ptr(), lens.data_ptr()
    sel, nlines = ugrep_amd.select_lines(bp, n, sp, lp, m, False, stream=sptr)
    rec = torch.empty((3, max(sel, 1)), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def step():
        a = ugrep_amd.select_lines(bp, n, sp, lp, m, False, rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(),
                                   sel, sptr)
        b = ugrep_amd.select_lines(bp, n, sp, lp, m, False, stream=sptr)
        c = ugrep_amd.select_lines(bp, n, sp, lp, m, True, stream=sptr)
        return a, b, c

    (a, b, c), _ = timed(step)
    _, t_write = timed(lambda: ugrep_amd.select_lines(bp, n, sp, lp, m, False, rec[0].data_ptr(), rec[1].data_ptr(),
                                                      rec[2].data_ptr(), sel, sptr))
    _, t_count = timed(lambda: ugrep_amd.select_lines(bp, n, sp, lp, m, False, stream=sptr))
    _, t_inv = timed(lambda: ugrep_amd.select_lines(bp, n, sp, lp, m, True, stream=sptr))
    (nl, ml), t_lines = timed(lambda: ugrep_amd.lines(bp, n, sp, m, 0, sptr))
    # sanity (not timed): records ascending, every span ends on a newline or at len, counts add up
    nl_torch = int((buf[:n] == 10).sum().item())
    asc = bool((rec[2, 1:sel] > rec[2, :sel - 1]).all().item()) if sel > 1 else True
    ends = rec[1, :sel]
    ends_ok = bool(((buf[ends.clamp(max=n - 1)] == 10) | (ends == n)).all().item()) if sel else True
    alg = n + 12 * m + 24 * sel  # every byte read once + a 12-byte match read + a 24-byte record written
    print(json.dumps({
        "what": "ugpu_select_lines (line records of the matching lines; count-only; inverted count-only)",
        "config": args.config, "bytes": n, "matches": m, "lines": nlines, "selected": sel,
        "selected_inverted": c[0], "newlines": nl, "matching_lines": ml,
        "counts_ok": a == b == (sel, nlines) and c[1] == nlines and sel + c[0] == nlines
        and nlines - nl_torch in (0, 1),
        "records_ascending": asc, "ends_ok": ends_ok,
        "ms_write_call": round(t_write * 1e3, 4), "ms_count_call": round(t_count * 1e3, 4),
        "ms_inverted_count_call": round(t_inv * 1e3, 4), "ms_ugpu_lines_count_call": round(t_lines * 1e3, 4),
        "GBps_input_write_call": round(n / t_write / 1e9, 1),
        "GBps_algorithmic_write_call": round(alg / t_write / 1e9, 1), "algorithmic_bytes": alg}), flush=True)


if __name__ == "__main__":
    main()
