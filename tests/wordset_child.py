"""Child process of tests/test_wordset.py: scans the shared inputs with the
environment the parent set (UGPU_MAX_GRID, UGPU_NG) and prints one JSON line
{input name: {"plain": [count, digest, dcap, triples hash], "word": ...}} and
the kernel ids.  The knobs are read when tables and scanners are created, so a
fresh process sees exactly one setting."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def triples_hash(trip):
    return hashlib.sha256(json.dumps(trip, separators=(",", ":")).encode()).hexdigest()[:16]


def main():
    import ugrep_amd as U
    import wordset_gen
    n, inputs = wordset_gen.child_inputs(sys.argv[1])
    opc = U.compile_regex(wordset_gen.regex(wordset_gen.words(n)))
    out = {"kernel": {}}
    for mode, word in (("plain", False), ("word", True)):
        pat = U.Pattern(opc, word=word)
        out["kernel"][mode] = pat.info()["kernel"]
        for name, buf in inputs:
            r = U.find_all(pat, buf.tobytes(), offsets=True)
            out.setdefault(name, {})[mode] = [r.count, r.digest, r.dcap, triples_hash(r.triples())]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
