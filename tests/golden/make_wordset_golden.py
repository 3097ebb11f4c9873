#!/usr/bin/env python3
"""Generate tests/golden/wordset_cases.json: reference results for large
string sets (ugrep -f words.txt, long alternations), the inputs of the n-gram
kernel (kernel 7), from the reference harness (oracle/_ref/ref_harness:
libreflex compiled from the reference sources).

Sets: the first 100, 300 and 1000 words of tests/wordset_gen.py's seeded
sequence; the 100-word set under -i; the 300-word set under option W (modes
reUW and reW).  Inputs: an edge text around the set's words (full match
list) and the gen:K:5:0:262144 corpora (count, digest, dcap).  The reference's
opcode words are stored for sets up to 300 words; the 1000-word case keeps the
seed and the totals and is compiled natively by the tests.

Build container only; the output is data, committed."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
import wordset_gen  # noqa: E402

HARNESS = os.path.join(REPO, "oracle", "_ref", "ref_harness")
GOLDEN = os.path.join(REPO, "tests", "golden")

# (name, words, mode, icase)
CASES = [("w100", 100, "re", False), ("w300", 300, "re", False), ("w1000", 1000, "re", False),
         ("w100i", 100, "re", True), ("w300_reUW", 300, "reUW", False), ("w300_reW", 300, "reW", False)]


def run(args):
    r = subprocess.run([HARNESS] + args, capture_output=True)
    if r.returncode:
        raise SystemExit("harness failed: %s\n%s" % (args[:2], r.stderr.decode()[-400:]))
    return r.stdout.decode()


def main():
    cases = []
    for name, n, mode, icase in CASES:
        ws = wordset_gen.words(n)
        rx = ("(?i)" if icase else "") + wordset_gen.regex(ws)
        edge = wordset_gen.edge_text(ws)
        ins = [("edge", "hex:" + edge.hex(), True)]
        for kind in (1, 3, 4):
            ins.append(("gen%d_256k" % kind, "gen:%d:5:0:262144" % kind, False))
        opc = None
        if n <= 300:
            opc = json.loads(run(["dump", mode.rstrip("W"), rx]))["opc"]
        res = []
        for iname, spec, full in ins:
            lines = run(["find", mode, rx, spec] + (["list"] if full else [])).strip().split("\n")
            cnt, dg, dc = (int(x) for x in lines[0].split())
            lst = [[int(v) for v in ln.split()] for ln in lines[1:]] if full else None
            res.append(dict(input=iname, spec=spec if not full else None, count=cnt, digest=dg, dcap=dc, list=lst))
        cases.append(dict(name=name, words=n, seed=wordset_gen.SEED, mode=mode, icase=icase, opc=opc, results=res))
    out = os.path.join(GOLDEN, "wordset_cases.json")
    with open(out, "w") as f:
        json.dump(dict(cases=cases), f, separators=(",", ":"))
    print("%d cases -> %s (%d bytes)" % (len(cases), out, os.path.getsize(out)), file=sys.stderr)


if __name__ == "__main__":
    main()
