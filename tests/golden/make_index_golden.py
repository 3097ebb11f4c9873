#!/usr/bin/env python3
"""Writes tests/golden/index_cases.json from the reference indexer.

    python3 tests/golden/make_index_golden.py REFERENCE_DIR [--time OUT.json]

Compiles ugrep-indexer from the reference's sources (no zlib) into a temporary
directory, which is removed again, runs it over the inputs of
tests/index_model.py at all ten accuracies with and without -I, and records
per input, accuracy and -I: the header byte, the table's length, the table
(its bytes, once per distinct table, when it has at most 4096; its SHA-256
beyond) and the noise percent that -v prints.  Also recorded: the whole store of a
one-file directory.  --time measures the indexer (one thread) on the three
shapes of tools/bench_index.py and writes the seconds to OUT.json."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import index_model as im  # noqa: E402

SOURCES = ["src/ugrep-indexer.cpp", "src/glob.cpp", "lib/input.cpp", "lib/utf8.cpp", "lib/error.cpp", "lib/debug.cpp"]
DEFINES = ["-DWITH_NO_INDENT", "-DHAVE_STRUCT_DIRENT_D_TYPE", "-DHAVE_STRUCT_DIRENT_D_INO"]
ONE_FILE = ("notes.txt", b"one file, one record\nin this store\n")


def build(ref, tmp):
    exe = os.path.join(tmp, "ugrep-indexer")
    subprocess.check_call(["g++", "-O2", "-std=c++11"] + DEFINES + ["-I" + os.path.join(ref, "include"),
                          "-I" + os.path.join(ref, "src")] + [os.path.join(ref, s) for s in SOURCES] +
                          ["-o", exe, "-lpthread"])
    return exe


def run(exe, d, accuracy, ignore_binary):
    """Indexes directory d afresh: ({name: (header, table)}, {name: percent})"""
    store = os.path.join(d, im.STORE_NAME)
    if os.path.exists(store):
        os.remove(store)
    args = [exe, "-%d" % accuracy, "-v", "-f"] + (["-I"] if ignore_binary else []) + [d]
    out = subprocess.run(args, stdout=subprocess.PIPE, check=True, cwd=d, env={"HOME": d}).stdout.decode()
    with open(store, "rb") as f:
        recs = {nm.decode(): (h, t) for nm, acc, h, t in im.parse_store(f.read()) if acc == accuracy}
    pct = {}
    for line in out.splitlines():
        m = re.match(r"^[ BICA]\s*\d+\s*(\d+)% (.*)$", line)
        if m:
            pct[os.path.basename(m.group(2))] = int(m.group(1))
    return recs, pct


def golden(exe, tmp):
    d = os.path.join(tmp, "cases")
    os.mkdir(d)
    inputs = im.golden_inputs()
    for name, _, data in inputs:
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    tables, cases = [], []
    results = {(a, ib): run(exe, d, a, ib) for a in range(10) for ib in (False, True)}
    for name, spec, _ in inputs:
        rows = []
        for a in range(10):
            for ib in (False, True):
                recs, pct = results[a, ib]
                h, t = recs[name]
                # the table: its place in "tables" when it has at most 4096 bytes, its SHA-256 beyond
                ref = "" if not t else im.table_sha(t)
                if t and len(t) <= 4096:
                    if t.hex() not in tables:
                        tables.append(t.hex())
                    ref = tables.index(t.hex())
                rows.append([a, int(ib), h, len(t), ref, pct.get(name, 0)])
        cases.append({"name": name, "input": spec, "rows": rows})
    one = os.path.join(tmp, "one")
    os.mkdir(one)
    with open(os.path.join(one, ONE_FILE[0]), "wb") as f:
        f.write(ONE_FILE[1])
    run(exe, one, 4, False)
    with open(os.path.join(one, im.STORE_NAME), "rb") as f:
        store = f.read()
    doc = {"rows": ["accuracy", "ignore_binary", "header", "table_len", "table (index into tables, or SHA-256)", "noise_percent"],
           "cases": cases, "tables": tables,
           "one_file_store": {"name": ONE_FILE[0], "input_hex": ONE_FILE[1].hex(), "accuracy": 4,
                              "store_hex": store.hex()}}
    path = os.path.join(HERE, "index_cases.json")
    with open(path, "w") as f:
        # one case and one table per line
        def d(x):
            return json.dumps(x, separators=(",", ":"))
        f.write('{"rows":%s,\n"cases":[\n%s],\n"tables":[\n%s],\n"one_file_store":%s}\n'
                % (d(doc["rows"]), ",\n".join(map(d, cases)), ",\n".join(map(d, tables)), d(doc["one_file_store"])))
    print("%s: %d cases, %d tables, %d bytes" % (path, len(cases), len(tables), os.path.getsize(path)))


def timing(exe, tmp, out):
    """The indexer's wall time (page cache warm, one thread) on the bench shapes."""
    res = {}
    pool = im.bench_pool()
    for label, count, size in (("1x1GiB", 1, 1 << 30), ("4096x256KiB", 4096, 256 << 10), ("65536x1KiB", 65536, 1 << 10)):
        d = os.path.join(tmp, label)
        os.mkdir(d)
        for i in range(count):
            with open(os.path.join(d, "f%06d" % i), "wb") as f:
                f.write(im.bench_input(pool, i, size))
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            subprocess.run([exe, "-4", "-f", "-q", d], check=True, cwd=d, env={"HOME": d}, stdout=subprocess.DEVNULL)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        res[label] = {"seconds": best, "bytes": count * size, "gb_per_s": count * size / best / 1e9, "threads": 1}
        shutil.rmtree(d)
        print(label, res[label])
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ref = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref, tmp)
        if len(sys.argv) > 3 and sys.argv[2] == "--time":
            timing(exe, tmp, sys.argv[3])
        else:
            golden(exe, tmp)


if __name__ == "__main__":
    main()
