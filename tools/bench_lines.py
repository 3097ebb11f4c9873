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

--bool K times Boolean line queries (ugpu_select_lines_bool) on
the same corpus: K match lists from K different needle patterns (three random
three-letter words each, the first is the config's own), one CNF that uses
every list; per step one count-only call and one call that writes the records.
In the same run it times the K count-only ugpu_select_lines calls a caller
needs without the fused pass (one per list; the K line lists would still have
to be copied and combined on the host, which is not timed).

--columns times ugpu_columns on the match starts: per step one
ugpu_columns call with all three outputs and one ugpu_lines call on the same
list, alternating, each timed on its own; then the same with ugpu_lines held to
its dense assign pass (UGPU_LINES_MODE=1), the pass ugpu_columns' assign pass
corresponds to.  Algorithmic bytes of ugpu_columns: the buffer twice plus 8 B
read and 24 B written per position.  A kernel trace of the run gives
col_summary_kernel / col_assign_kernel beside nl_count_kernel / nl_assign_kernel.
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
    ap.add_argument("--bool", type=int, default=0, metavar="K", dest="nbool",
                    help="time ugpu_select_lines_bool over K match lists (1..16)")
    ap.add_argument("--columns", action="store_true", help="time ugpu_columns beside ugpu_lines")
    ap.add_argument("--tab", type=int, default=8, help="--columns: the tab size")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
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
    if args.nbool:
        return boolean(args, dev, sptr, buf, n, opc)
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
    if args.columns:
        return columns(args, dev, sptr, buf, n, starts, m)
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


def columns(args, dev, sptr, buf, n, starts, m):
    bp, sp = buf.data_ptr(), starts.data_ptr()
    out = torch.empty((3, max(m, 1)), dtype=torch.int64, device=dev)
    lines = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def alternate():
        """(s per ugpu_columns call, s per ugpu_lines call), one of each per step"""
        tc = tl = 0.0
        for i in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ugrep_amd.columns(bp, n, sp, m, args.tab, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), sptr)
            t1 = time.perf_counter()
            ugrep_amd.lines(bp, n, sp, m, lines.data_ptr(), sptr)
            t2 = time.perf_counter()
            if i >= args.warmup:
                tc, tl = tc + t1 - t0, tl + t2 - t1
        return tc / args.steps, tl / args.steps

    t_col, t_lines = alternate()
    os.environ["UGPU_LINES_MODE"] = "1"
    t_col2, t_dense = alternate()
    del os.environ["UGPU_LINES_MODE"]
    # sanity (not timed): the lines are ugpu_lines', a line begins behind a newline, the column is within the line
    col, bol, line = out[0, :m], out[1, :m], out[2, :m]
    st = starts[:m]
    ok = bool((line == lines[:m]).all().item()) and bool(((bol == 0) | (buf[(bol - 1).clamp(min=0)] == 10)).all().item()) \
        and bool(((bol <= st) & (col >= 0) & (col <= (st - bol) * args.tab)).all().item())
    alg = 2 * n + 32 * m  # the buffer twice + a position read and three values written per position
    res = {
        "what": "ugpu_columns (column, line begin and line of every match start) beside ugpu_lines, alternating",
        "config": args.config, "bytes": n, "positions": m, "tab": args.tab, "outputs_ok": ok,
        "ms_columns_call": round(t_col * 1e3, 4), "ms_lines_call": round(t_lines * 1e3, 4),
        "ms_columns_call_2": round(t_col2 * 1e3, 4), "ms_lines_dense_call": round(t_dense * 1e3, 4),
        "GBps_input_columns_call": round(n / t_col / 1e9, 1),
        "GBps_algorithmic_columns_call": round(alg / t_col / 1e9, 1), "algorithmic_bytes": alg,
        "max_column": int(col.max().item()) if m else 0}
    text = json.dumps(res)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


NEEDLES = ["qux|zot|wib", "mep|dak|yol", "vug|hix|pym", "kob|raz|tew", "jid|nuf|gax", "lev|sop|cuz", "wam|biq|fyr",
           "hod|zim|kep", "tuv|goj|nac", "pel|rix|dub", "sab|myk|vot", "cer|luh|zan", "fip|gow|jyt", "bux|dor|nim",
           "yag|teq|hul"]


def match_list(pat, dev, sptr, buf, n):
    sc = ugrep_amd.Scanner(pat)
    sc.scan(buf.data_ptr(), 0, n, n, True, 0, sptr)
    m = sc.totals().count
    starts = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    lens = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    caps = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    sc.offsets(starts.data_ptr(), lens.data_ptr(), caps.data_ptr(), m, sptr)
    torch.cuda.synchronize(dev)
    sc.close()
    return starts, lens, m


def boolean(args, dev, sptr, buf, n, opc):
    k = args.nbool
    if not 1 <= k <= 16:
        sys.exit("--bool takes 1..16 lists")
    pats = [ugrep_amd.Pattern(opc)] + [ugrep_amd.Pattern(ugrep_amd.compile_regex(rx)) for rx in NEEDLES[:k - 1]]
    found = [match_list(p, dev, sptr, buf, n) for p in pats]
    lists = [(s.data_ptr(), ln.data_ptr(), m) for s, ln, m in found]
    # (list 0 or list 1) and, for every later list t: not t (t even), t or list 0 (t odd)
    clauses = [(3 if k > 1 else 1, 0)] + [((1 << t | 1, 0) if t & 1 else (0, 1 << t)) for t in range(2, k)]
    bp = buf.data_ptr()

    def timed(fn):
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize(dev)
        return out, (time.perf_counter() - t0) / args.steps

    sel, nlines, _ = ugrep_amd.select_lines_bool(bp, n, lists, clauses, stream=sptr)
    rec = torch.empty((3, max(sel, 1)), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    cnt, t_count = timed(lambda: ugrep_amd.select_lines_bool(bp, n, lists, clauses, stream=sptr))
    wrt, t_write = timed(lambda: ugrep_amd.select_lines_bool(bp, n, lists, clauses, False, False, rec[0].data_ptr(),
                                                             rec[1].data_ptr(), rec[2].data_ptr(), sel, sptr))
    fil, t_files = timed(lambda: ugrep_amd.select_lines_bool(bp, n, lists, clauses, False, True, stream=sptr))
    sep, t_sep = timed(lambda: [ugrep_amd.select_lines(bp, n, s, ln, m, False, stream=sptr) for s, ln, m in lists])
    # sanity (not timed): each list alone through the fused call gives select_lines' count; records ascending
    alone = [ugrep_amd.select_lines_bool(bp, n, lists, [(1 << t, 0)], stream=sptr)[0] for t in range(k)]
    asc = bool((rec[2, 1:sel] > rec[2, :sel - 1]).all().item()) if sel > 1 else True
    mtot = sum(m for _, _, m in lists)
    res = {
        "what": "ugpu_select_lines_bool (count-only; record write; --files count-only) against K count-only "
                "ugpu_select_lines calls",
        "config": args.config, "bytes": n, "lists": k, "matches": [m for _, _, m in lists],
        "clauses": [list(c) for c in clauses], "lines": nlines, "selected": sel, "selected_files": fil[0],
        "counts_ok": cnt == wrt == (sel, nlines, sel > 0) and alone == [x[0] for x in sep]
        and all(x[1] == nlines for x in sep) and sel <= nlines,
        "records_ascending": asc,
        "ms_bool_count_call": round(t_count * 1e3, 4), "ms_bool_write_call": round(t_write * 1e3, 4),
        "ms_bool_files_count_call": round(t_files * 1e3, 4),
        "ms_separate_count_calls": round(t_sep * 1e3, 4),
        "separate_over_bool_count": round(t_sep / t_count, 2),
        # buffer passes: newline count + select-count (+ select-write); each separate call is newline count + select-count
        "bytes_read_bool_count_call": 2 * n + 2 * 12 * mtot,
        "bytes_read_bool_write_call": 3 * n + 3 * 12 * mtot,
        "bytes_read_separate_count_calls": 2 * n * k + 2 * 12 * mtot,
        "bytes_written_bool_write_call": 24 * sel}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
