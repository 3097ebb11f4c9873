#!/usr/bin/env python3
"""Writes tests/golden/hfa_cases.json from the reference CLI's index query.

    python3 tests/golden/make_hfa_golden.py [UGREP]

UGREP is the reference ugrep (default: oracle/_ref/ugrep, which build() makes
where the reference's sources are).  A seeded corpus (hfa_model.corpus) is
written into a temporary directory with a ._UG#_Store from tests/index_model.py
(tied to the reference indexer by index_cases.json), the files' times set
before the store's.  For every pattern and the accuracies 0, 4 and 9 it runs
ugrep -rl PATTERN and ugrep --index=log -rl PATTERN and records the files the
log names (kept: their tables passed Pattern::match_hfa) and the files that
match.  A pattern without an HFA prints no log line and searches every file:
its rows keep every file and say index_off.  The corpus is recorded by its specification, not its bytes.

Asserted before anything is written: the indexed search lists the same files
as the plain one; no log line says (changed) or (not indexed); over all
(pattern, accuracy, file) triples at least a fifth are kept and at least a
fifth are skipped."""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hfa_model as hm  # noqa: E402
import index_model as im  # noqa: E402

ACCURACIES = (0, 4, 9)


def run(ugrep, d, args):
    r = subprocess.run([ugrep] + args + ["."], cwd=d, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120,
                       env={"HOME": d, "PATH": os.environ.get("PATH", "")})
    assert r.returncode in (0, 1), (args, r.stderr[-500:])
    return sorted(os.path.normpath(x) for x in r.stdout.decode().split("\n") if x), r.stderr.decode()


def main():
    ugrep = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref",
                                                               "ugrep")
    corpus = hm.corpus()
    patterns = hm.patterns()
    files = [(c["name"], hm.corpus_bytes(c)) for c in corpus]
    names = sorted(nm for nm, _ in files)
    rows = []
    kept_n = total_n = 0
    for acc in ACCURACIES:
        with tempfile.TemporaryDirectory() as d:
            recs = []
            old = time.time() - 1000
            for nm, data in files:
                with open(os.path.join(d, nm), "wb") as f:
                    f.write(data)
                os.utime(os.path.join(d, nm), (old, old))
                h, t, _ = im.index_record(data, acc)
                recs.append((nm, h, t))
            with open(os.path.join(d, im.STORE_NAME), "wb") as f:
                f.write(im.store_bytes(recs, acc))
            for pi, p in enumerate(patterns):
                args = p["args"] + ["-e", p["pattern"]]
                want, _ = run(ugrep, d, ["-rl"] + args)
                got, log = run(ugrep, d, ["--index=log", "-rl"] + args)
                assert got == want, (p, acc, got, want)
                assert "(changed)" not in log and "(not indexed)" not in log, log
                kept = sorted(os.path.normpath(ln[len("INDEX LOG: "):].split(" (")[0]) for ln in log.splitlines()
                              if ln.startswith("INDEX LOG: "))
                row = {"pattern": pi, "accuracy": acc, "kept": kept, "match": want}
                if want and not kept:
                    # no log line although files match: the pattern has no HFA (src/ugrep.cpp:8931), the
                    # index is off and every file is searched
                    kept = row["kept"] = names
                    row["index_off"] = True
                assert set(want) <= set(kept) <= set(names), (p, acc)
                rows.append(row)
                kept_n += len(kept)
                total_n += len(names)
    assert 5 * kept_n >= total_n and 5 * (total_n - kept_n) >= total_n, (kept_n, total_n)
    out = {"corpus": corpus, "patterns": patterns, "rows": rows, "kept": kept_n, "triples": total_n}
    with open(os.path.join(HERE, "hfa_cases.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%d patterns, %d files, %d of %d triples kept" % (len(patterns), len(names), kept_n, total_n))


if __name__ == "__main__":
    main()
