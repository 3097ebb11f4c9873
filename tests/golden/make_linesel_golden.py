#!/usr/bin/env python3
"""Regenerate tests/golden/linesel_cases.json (run in the build container only).

Line-selection goldens from the REFERENCE's own recorded CLI outputs
(/root/reference/tests/out/Hello_*.out, produced by tests/verify.sh over
Hello.* empty.txt emptyline.txt) and its matcher (oracle/_ref/ref_harness, as
make_golden.py):

  per (file, pattern): the reference's match list (start, len), the printed
  (lineno, kind) list of -n, -nv, -nC2 and -nvC2 (kind 1 = selected, separator
  ':' or '|'; kind 0 = context, separator '-') and, for the patterns whose
  matches cannot hold a newline (Hello, nomatch), the -c / -cv counts.

The empty pattern (Hello_-n.out: every line prints) has no harness list: its
matches are derived, a zero-length match at every line start.

The input files are tests/golden/verify/.  Only the JSON is committed.

Usage: make -C oracle ref && python tests/golden/make_linesel_golden.py
"""
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
HARNESS = os.path.join(REPO, "oracle", "_ref", "ref_harness")
REFOUT = "/root/reference/tests/out"

FILES = ["Hello.java", "Hello.sh", "Hello.bat", "Hello.txt", "empty.txt", "emptyline.txt"]
# output name -> (patterns.json key or None, harness mode, regex)
PATTERNS = {
    "Hello": ("hello", "reU", "Hello"),
    "wnhS": ("hello_wnhS", "reU", r"\w+[\n\h]+\S+"),
    "SnS": (None, "reU", r"\S\n\S"),
    "nomatch": ("nomatch", "reU", "nomatch"),
}
OPTIONS = ["-n", "-nv", "-nC2", "-nvC2"]
COUNTED = ("Hello", "nomatch")  # -c / -cv equal the printed line counts only without '\n' in a match

STRIP = re.compile(r"\x1b\[[0-9;]*[mK]")
LINE = re.compile(r"^([A-Za-z0-9_.]+)([:|-])(\d+)([:|-])")
COUNT = re.compile(r"^([A-Za-z0-9_.]+):(\d+)$")


def read_out(name):
    with open(os.path.join(REFOUT, name), encoding="latin-1") as f:
        return [STRIP.sub("", ln.rstrip("\n")) for ln in f]


def printed(name):
    """file -> [[lineno, kind], ...] of one recorded output."""
    out = {f: [] for f in FILES}
    for ln in read_out(name):
        if ln.startswith("Binary file"):
            continue
        m = LINE.match(ln)
        if not m:
            sys.exit("%s: cannot parse %r" % (name, ln))
        if m.group(1) in out:
            out[m.group(1)].append([int(m.group(3)), 0 if m.group(4) == "-" else 1])
    return out


def counts(name):
    out = {}
    for ln in read_out(name):
        m = COUNT.match(ln)
        if m and m.group(1) in FILES:
            out[m.group(1)] = int(m.group(2))
    return out


def find(mode, rx, path):
    out = subprocess.check_output([HARNESS, "find", mode, rx, "file:" + path, "list"]).decode().split("\n")
    return [[int(v) for v in ln.split()[:2]] for ln in out[1:] if ln.strip()]


def main():
    if not os.path.exists(HARNESS):
        sys.exit("build the reference harness first: make -C oracle ref")
    cases = []
    for oname, (pkey, mode, rx) in PATTERNS.items():
        prints = {opt: printed("Hello_%s%s.out" % (oname, opt)) for opt in OPTIONS}
        cnt = {opt: counts("Hello_%s%s.out" % (oname, opt)) for opt in ("-c", "-cv")} if oname in COUNTED else None
        for f in FILES:
            case = dict(file=f, pattern=oname, patterns_key=pkey, mode=mode, regex=rx, derived=False,
                        matches=find(mode, rx, os.path.join(HERE, "verify", f)),
                        printed={opt: prints[opt][f] for opt in OPTIONS})
            if cnt:
                case["counts"] = {opt: cnt[opt][f] for opt in ("-c", "-cv")}
            cases.append(case)
    # the empty pattern: every line prints; derived zero-length matches at the line starts
    prints = printed("Hello_-n.out")
    for f in FILES:
        data = open(os.path.join(HERE, "verify", f), "rb").read()
        starts = [0] if data else []
        starts += [i + 1 for i, b in enumerate(data) if b == 10 and i + 1 < len(data)]
        cases.append(dict(file=f, pattern="", patterns_key=None, mode=None, regex="", derived=True,
                          matches=[[s, 0] for s in starts], printed={"-n": prints[f]}))
    with open(os.path.join(HERE, "linesel_cases.json"), "w") as fh:
        json.dump(dict(source="tests/out/Hello_{Hello,wnhS,SnS,nomatch}{-n,-nv,-nC2,-nvC2,-c,-cv}.out, Hello_-n.out",
                       files=FILES, cases=cases), fh, indent=1)
    print("cases", len(cases))


if __name__ == "__main__":
    main()
