#!/usr/bin/env python3
"""Regenerate tests/golden/columns_cases.json and tests/golden/columns_mix.bin
(run in the build container only).

Column goldens (ugrep -k / --tabs) from the REFERENCE:

  recorded  the (file, line, column, offset) rows of its own recorded CLI
            outputs /root/reference/tests/out/Hello_{Hello,wnhS,SnS}--csv-onkb.out
            (tests/verify.sh over Hello.* with the default --tabs=8), for the
            files in tests/golden/verify/ (checked to equal the reference's);
  mix       the (line, column, offset) rows of
            oracle/_ref/ugrep --csv -onkb --tabs=N x tests/golden/columns_mix.bin
            for N = 1, 2, 4, 8.  columns_mix.bin is written here from a fixed
            seed: units drawn from a b \\t \\n \\r e-acute euro 0xFF 0x80 x, one
            line of 9000 bytes without a tab, and one line of 4096 tabs with an
            x behind them (so that a reference row stands at column 32769).

line and column are as printed: 1-based.  Only the JSON and columns_mix.bin
are committed.

Usage: make -C oracle ref && python tests/golden/make_columns_golden.py
"""
import json
import os
import random
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
UGREP = os.path.join(REPO, "oracle", "_ref", "ugrep")
REFTESTS = "/root/reference/tests"
MIX = os.path.join(HERE, "columns_mix.bin")

# output name -> patterns.json key (None: no table of that pattern is committed)
PATTERNS = {"Hello": "hello", "wnhS": "hello_wnhS", "SnS": None}
ROW = re.compile(r'^(?:"([^"]+)",)?(\d+),(\d+),(\d+),')
UNITS = [b"a", b"b", b"\t", b"\n", b"\r", "é".encode(), "€".encode(), b"\xff", b"\x80", b"x"]


def make_mix():
    rng = random.Random(20240611)

    def units(n, pool=UNITS):
        return b"".join(rng.choice(pool) for _ in range(n))

    notab = [u for u in UNITS if u not in (b"\t", b"\n")]
    long_line = b""
    while len(long_line) < 9000:
        long_line += rng.choice(notab)
    long_line = long_line[:8999] + b"x"       # (a cut character leaves continuation bytes: they count 0)
    data = units(2200) + b"\n" + long_line + b"\n" + units(2200) + b"\n" + b"\t" * 4096 + b"x\n" + units(2200)
    assert len(data) <= 24 << 10, len(data)
    with open(MIX, "wb") as f:
        f.write(data)
    return data


def rows_of(text, with_file):
    out = []
    for ln in text.split("\n"):
        if not ln:
            continue
        m = ROW.match(ln)
        if not m or bool(m.group(1)) != with_file:
            sys.exit("cannot parse %r" % ln)
        r = [int(m.group(2)), int(m.group(3)), int(m.group(4))]
        out.append([m.group(1)] + r if with_file else r)
    return out


def main():
    if not os.path.exists(UGREP):
        sys.exit("build the reference CLI first: make -C oracle ref")
    recorded = []
    for oname, pkey in PATTERNS.items():
        with open(os.path.join(REFTESTS, "out", "Hello_%s--csv-onkb.out" % oname), encoding="latin-1") as f:
            rows = rows_of(f.read(), True)
        for name in sorted({r[0] for r in rows}):
            ours = open(os.path.join(HERE, "verify", name), "rb").read()
            assert ours == open(os.path.join(REFTESTS, name), "rb").read(), name
        recorded.append(dict(pattern=oname, patterns_key=pkey, tab=8, rows=rows))
    make_mix()
    mix = {}
    for tab in (1, 2, 4, 8):
        out = subprocess.run([UGREP, "--csv", "-onkb", "--tabs=%d" % tab, "x", MIX], stdout=subprocess.PIPE,
                             check=True).stdout.decode("latin-1")
        mix[str(tab)] = rows_of(out, False)
    with open(os.path.join(HERE, "columns_cases.json"), "w") as fh:
        json.dump(dict(source="tests/out/Hello_{Hello,wnhS,SnS}--csv-onkb.out; ugrep --csv -onkb --tabs=N x columns_mix.bin",
                       recorded=recorded, mix=dict(file="columns_mix.bin", pattern="x", rows=mix)), fh,
                  separators=(",", ":"))
    print("recorded rows", sum(len(c["rows"]) for c in recorded), "mix rows", {k: len(v) for k, v in mix.items()})


if __name__ == "__main__":
    main()
