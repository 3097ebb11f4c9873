#!/usr/bin/env python3
"""Regenerate tests/golden/boolsel_cases.json (run in the build container only).

Boolean line-query goldens from the REFERENCE CLI (oracle/_ref/ugrep, built by
make -C oracle ref) over tests/golden/verify/{Hello.java,.sh,.bat,.txt,
empty.txt,emptyline.txt}: the ten --bool queries of the reference's own CLI
suite (tests/verify.sh:354) and its three option forms (:368-378).

  per (query, file): the printed (lineno, kind) list of
      ugrep -U -n [--files] [-C2] --bool Q FILE
  (kind 1 = selected, separator ':'; kind 0 = context, separator '-'), the
  query's CNF over its sub-patterns (written by hand below), and the match
  list (start, len) of every sub-pattern from oracle/_ref/ref_harness find, so
  that the low-level tests need no compiler.

Cross-checks, each stopping the run: the per-file line counts against the
reference's recorded tests/out/Hello_*--bool-c.out and *--files--bool-c.out
(--files leaves a file out of -c when its formula fails), and the option
forms against the line counts of tests/out/Hello--and*.out.

Only the JSON is committed.

Usage: make -C oracle ref && python tests/golden/make_boolsel_golden.py
"""
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
HARNESS = os.path.join(REPO, "oracle", "_ref", "ref_harness")
UGREP = os.path.join(REPO, "oracle", "_ref", "ugrep")
REFOUT = "/root/reference/tests/out"

FILES = ["Hello.java", "Hello.sh", "Hello.bat", "Hello.txt", "empty.txt", "emptyline.txt"]

# (name, CLI arguments, sub-patterns, clauses (pos, neg) over them, recorded-output stem or None)
H, W, B, G = "Hello", "World", "bin", "greeting"
QUERIES = [
    ("", ["--bool", ""], [], []),
    ("Hello World", ["--bool", "Hello World"], [H, W], [(1, 0), (2, 0)]),
    ("Hello -World", ["--bool", "Hello -World"], [H, W], [(1, 0), (0, 2)]),
    ("Hello -bin", ["--bool", "Hello -bin"], [H, B], [(1, 0), (0, 2)]),
    ("bin -Hello", ["--bool", "bin -Hello"], [B, H], [(1, 0), (0, 2)]),
    ("bin -greeting", ["--bool", "bin -greeting"], [B, G], [(1, 0), (0, 2)]),
    ("Hello -World|greeting", ["--bool", "Hello -World|greeting"], [H, W, G], [(1, 0), (4, 2)]),
    ("Hello -bin|greeting", ["--bool", "Hello -bin|greeting"], [H, B, G], [(1, 0), (4, 2)]),
    ("Hello -(greeting|World)", ["--bool", "Hello -(greeting|World)"], [H, G, W], [(1, 0), (0, 2), (0, 4)]),
    ('"a Hello" greeting', ["--bool", '"a Hello" greeting'], ["\\Qa Hello\\E", G], [(1, 0), (2, 0)]),
]
OPTION_FORMS = [
    ("-e Hello --and World", ["-e", H, "--and", W], [H, W], [(1, 0), (2, 0)], "Hello--and.out"),
    ("-e Hello --andnot World", ["-e", H, "--andnot", W], [H, W], [(1, 0), (0, 2)], "Hello--andnot.out"),
    ("-e Hello --and --not World -e greeting", ["-e", H, "--and", "--not", W, "-e", G], [H, W, G],
     [(1, 0), (4, 2)], "Hello--and--not.out"),
]
MODES = {"-n": [], "-n --files": ["--files"], "-nC2": ["-C2"], "-nC2 --files": ["--files", "-C2"]}

STRIP = re.compile(r"\x1b\[[0-9;]*[mK]")
LINE = re.compile(r"^([A-Za-z0-9_.]+)([:|-])(\d+)([:|-])")
COUNT = re.compile(r"^([A-Za-z0-9_.]+):(\d+)$")


def read_out(name):
    with open(os.path.join(REFOUT, name), encoding="latin-1") as f:
        return [STRIP.sub("", ln.rstrip("\n")) for ln in f]


def recorded_counts(name):
    out = {}
    for ln in read_out(name):
        m = COUNT.match(ln)
        if m and m.group(1) in FILES:
            out[m.group(1)] = int(m.group(2))
    return out


def run(args, mode, f):
    """[[lineno, kind], ...] the reference prints for one file."""
    cmd = [UGREP, "-U", "-n", "-H"] + MODES[mode] + args + [f]
    p = subprocess.run(cmd, cwd=os.path.join(HERE, "verify"), stdout=subprocess.PIPE)
    if p.returncode not in (0, 1):
        sys.exit("%r failed with %d" % (cmd, p.returncode))
    out = []
    for ln in p.stdout.decode("latin-1").split("\n"):
        if not ln or ln == "--":
            continue
        m = LINE.match(ln)
        if not m or m.group(1) != f:
            sys.exit("%r: cannot parse %r" % (cmd, ln))
        out.append([int(m.group(3)), 0 if m.group(4) == "-" else 1])
    return out


def find(rx, path):
    out = subprocess.check_output([HARNESS, "find", "reU", rx, "file:" + path, "list"]).decode().split("\n")
    return [[int(v) for v in ln.split()[:2]] for ln in out[1:] if ln.strip()]


def stem(query):
    return "Hello_" + re.sub(r"[^A-Za-z0-9_-]", "", query)


def main():
    for exe in (HARNESS, UGREP):
        if not os.path.exists(exe):
            sys.exit("build the reference first: make -C oracle ref")
    cases = []
    for name, args, patterns, clauses in QUERIES:
        want = {"-n": recorded_counts(stem(name) + "--bool-c.out"),
                "-n --files": recorded_counts(stem(name) + "--files--bool-c.out")}
        for f in FILES:
            printed = {mode: run(args, mode, f) for mode in MODES}
            for mode, cnt in want.items():
                got = sum(k for _, k in printed[mode])
                if got != cnt.get(f, 0):
                    sys.exit("%r %s %s: %d lines, the recorded -c says %s" % (name, mode, f, got, cnt.get(f)))
            cases.append(dict(query=name, bool=True, file=f, patterns=patterns, clauses=[list(c) for c in clauses],
                              matches=[find(rx, os.path.join(HERE, "verify", f)) for rx in patterns],
                              printed=printed))
    for name, args, patterns, clauses, recorded in OPTION_FORMS:
        lines = [ln.split(":", 1)[0] for ln in read_out(recorded) if ":" in ln]
        for f in FILES:
            printed = {mode: run(args, mode, f) for mode in MODES}
            if len(printed["-n"]) != lines.count(f):
                sys.exit("%r %s: %d lines, %s has %d" % (name, f, len(printed["-n"]), recorded, lines.count(f)))
            cases.append(dict(query=name, bool=False, file=f, patterns=patterns, clauses=[list(c) for c in clauses],
                              matches=[find(rx, os.path.join(HERE, "verify", f)) for rx in patterns],
                              printed=printed))
    with open(os.path.join(HERE, "boolsel_cases.json"), "w") as fh:
        json.dump(dict(source="oracle/_ref/ugrep -U -n -H [--files] [-C2] --bool Q FILE; counts checked against "
                              "tests/out/Hello_*--bool-c.out, *--files--bool-c.out, Hello--and*.out",
                       files=FILES, modes=sorted(MODES), cases=cases), fh, indent=1)
    print("cases", len(cases))


if __name__ == "__main__":
    main()
