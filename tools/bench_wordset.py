#!/usr/bin/env python3
"""Large string sets: the n-gram kernel (kernel 7) against the
kernels the same tables take with UGPU_NG=0 (dense_kernel for class tables,
wfind_kernel for wide tables and option W), in one process.

Corpus: the C2 word corpus (ugpu_gen UGPU_GEN_WORDS) resident in HBM.  Sets:
the first 100, 300, 1000 and 3000 words of tests/wordset_gen.py's seeded
sequence, plain and with option W.  Per set and option the tool builds the
table twice -- once as planned, once with UGPU_NG=0 in the environment while
the table and its scanner are created (the knob is read there) -- checks that
both give the same totals, and then times COUNT scans (ugpu_scan +
ugpu_scan_totals) and OFFSETS scans (+ ugpu_scan_offsets) of the two,
alternating them for --rounds rounds.  A leg whose UGPU_NG=0 kernel is
wfind_kernel scans --slow-bytes instead of --bytes (that kernel runs at well
under 1 % of HBM bandwidth: DESIGN §7).

--sweep: the crossover.  Over --sweep-bytes of the corpus, the 4-byte prefixes
of the 100-word set's words (a class table) are planted every 1/d bytes for each density d, so
that about d of all positions are true candidates whose walks go at least four
bytes deep, and both kernels are timed as above (COUNT).

Writes --out (profiles/wordset_ab.json): per leg the rounds of both variants
in ms, min / max, the speed-up of the medians, whether the n-gram kernel is
faster by more than the min-max spread of the UGPU_NG=0 rounds, and the
candidate fraction measured on the first 4 MiB (ugpu_ngram_candidates_host)
beside the host's estimate (prefilter_ppm).  Reads nothing outside the
repository."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

import ugrep_amd  # noqa: E402
import wordset_gen  # noqa: E402


def make(opc, word, ng):
    """(pattern, scanner) with UGPU_NG set as asked while both are created"""
    old = os.environ.pop("UGPU_NG", None)
    if not ng:
        os.environ["UGPU_NG"] = "0"
    try:
        pat = ugrep_amd.Pattern(opc, word=word)
        kernel = pat.info()["kernel"]
        sc = ugrep_amd.Scanner(pat, records=True)
    finally:
        os.environ.pop("UGPU_NG", None)
        if old is not None:
            os.environ["UGPU_NG"] = old
    return pat, sc, kernel


def count_ms(sc, buf, n, sptr):
    torch.cuda.synchronize()
    t = time.perf_counter()
    sc.scan(buf.data_ptr(), 0, n, n, True, 0, sptr)
    tot = sc.totals()
    return (time.perf_counter() - t) * 1e3, tot


def offsets_ms(sc, buf, n, sptr, out):
    torch.cuda.synchronize()
    t = time.perf_counter()
    sc.scan(buf.data_ptr(), 0, n, n, True, 0, sptr)
    tot = sc.totals()
    sc.offsets(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[0].numel(), sptr)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, tot


def summarize(a, b):
    return dict(ng_ms=a, ng0_ms=b, ng_min=min(a), ng_max=max(a), ng0_min=min(b), ng0_max=max(b),
                speedup=statistics.median(b) / statistics.median(a),
                faster_beyond_ng0_spread=max(a) < min(b) - (max(b) - min(b)))


def leg(opc, word, buf, n, sptr, rounds, offsets=True):
    pa, sa, ka = make(opc, word, True)
    pb, sb, kb = make(opc, word, False)
    _, ta = count_ms(sa, buf, n, sptr)  # (warm-up, and the equality check)
    _, tb = count_ms(sb, buf, n, sptr)
    same = (ta.count, ta.digest, ta.dcap) == (tb.count, tb.digest, tb.dcap)
    ca, cb, oa, ob = [], [], [], []
    for _ in range(rounds):
        ca.append(count_ms(sa, buf, n, sptr)[0])
        cb.append(count_ms(sb, buf, n, sptr)[0])
    res = dict(kernel_ng=ka, kernel_ng0=kb, bytes=n, matches=ta.count, same_totals=same,
               estimate_ppm=pa.info()["prefilter_ppm"], count=summarize(ca, cb))
    if offsets:
        m = max(ta.count, 1)
        out = (torch.empty(m, dtype=torch.int64, device=buf.device), torch.empty(m, dtype=torch.int32, device=buf.device),
               torch.empty(m, dtype=torch.int32, device=buf.device))
        for _ in range(rounds):
            oa.append(offsets_ms(sa, buf, n, sptr, out)[0])
            ob.append(offsets_ms(sb, buf, n, sptr, out)[0])
        res["offsets"] = summarize(oa, ob)
    res["count_tbps_ng"] = n / (statistics.median(ca) * 1e-3) / 1e12
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=16 << 30)
    ap.add_argument("--slow-bytes", type=int, default=128 << 20)
    ap.add_argument("--sizes", default="100,300,1000,3000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", default="1e-4,1e-3,1e-2,3e-2,1e-1", help="planted densities ('' = no sweep)")
    ap.add_argument("--sweep-bytes", type=int, default=1 << 30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wordset_ab.json"))
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("at least three rounds")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sptr = torch.cuda.current_stream(dev).cuda_stream
    n = args.bytes
    buf = torch.empty(n + 16, dtype=torch.uint8, device=dev)
    ugrep_amd.gen(ugrep_amd.GEN_WORDS, 1, 0, buf.data_ptr(), n, sptr)
    torch.cuda.synchronize()
    sample = buf[:4 << 20].cpu().numpy()
    result = dict(corpus="UGPU_GEN_WORDS seed 1", rounds=args.rounds, legs=[], sweep=[])
    for size in (int(s) for s in args.sizes.split(",") if s):
        opc = ugrep_amd.compile_regex(wordset_gen.regex(wordset_gen.words(size)))
        measured = float(ugrep_amd.host_ngram_candidates(opc, sample).mean())
        for word in (False, True):
            slow = ugrep_amd.host_plan(opc, word=word)["format"] == 2 or word
            ln = min(n, args.slow_bytes) if slow else n
            r = leg(opc, word, buf, ln, sptr, args.rounds)
            r.update(words=size, word=word, measured_candidate_fraction=measured)
            result["legs"].append(r)
            print(json.dumps(r), flush=True)
    if args.sweep:
        ws = wordset_gen.words(100)  # a class table: its UGPU_NG=0 kernel is dense_kernel
        opc = ugrep_amd.compile_regex(wordset_gen.regex(ws))
        pre = torch.tensor([list(w.encode("utf-8")[:4]) for w in ws], dtype=torch.uint8, device=dev)
        sn = min(n, args.sweep_bytes)
        for d in (float(x) for x in args.sweep.split(",")):
            ugrep_amd.gen(ugrep_amd.GEN_WORDS, 1, 0, buf.data_ptr(), sn, sptr)
            torch.cuda.synchronize()
            pos = torch.arange(7, sn - 16, max(int(round(1 / d)), 4), device=dev)
            which = torch.arange(pos.numel(), device=dev) % pre.shape[0]
            for j in range(4):
                buf[pos + j] = pre[which, j]
            torch.cuda.synchronize()
            measured = float(ugrep_amd.host_ngram_candidates(opc, buf[:4 << 20].cpu().numpy()).mean())
            for word in (False, True):
                ln = sn if not word else min(sn, args.slow_bytes)
                r = leg(opc, word, buf, ln, sptr, args.rounds, offsets=False)
                r.update(words=100, word=word, planted_density=d, measured_candidate_fraction=measured)
                result["sweep"].append(r)
                print(json.dumps(r), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
