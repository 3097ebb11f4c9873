"""Model of the batched FIND (ugpu_find_batch, ugpu_split_matches) in plain
numpy, and the fixture tables and inputs its tests share.

pack() is the packing rule of ugpu_find_batch; split() restates
ugpu_split_matches (include/ugpu.h) record by record.
"""
import json
import os

import numpy as np

from oracle_lib import GOLDEN

U64 = np.uint64

# input endings that meet the seam predicates (at_wb, at_we, at_eol, bol): a
# trailing newline, CR LF, '_', a word byte, a cut-off UTF-8 lead, two bytes of
# a three-byte sequence, and nothing.  (A bare '\r' is the exception: BARE_CR.)
ENDINGS = [b"", b"\n", b"\r\n", b"_", b"o", b"\xc3", b"\xe2\x82"]
BARE_CR = b"\r"


def pack(inputs):
    """(packed bytes as uint8, bounds as uint64 of len(inputs) + 1): the inputs
    back to back, a '\\n' added to each non-empty input that lacks it."""
    parts, bounds, off = [], [], 0
    for d in inputs:
        d = bytes(d)
        bounds.append(off)
        if d and not d.endswith(b"\n"):
            d += b"\n"
        parts.append(d)
        off += len(d)
    bounds.append(off)
    return np.frombuffer(b"".join(parts), np.uint8), np.asarray(bounds, U64)


def split(buf, bounds, start, length=None, cap=None, cap1=0):
    """ugpu_split_matches over host arrays: dict of first (nseg + 1), digest,
    dcap, newlines, mlines (nseg), rel and line (n; 0 for records outside
    [bounds[0], bounds[nseg]))."""
    buf = np.asarray(buf, np.uint8)
    bounds = np.asarray(bounds, U64)
    start = np.asarray(start, U64)
    n, nseg = start.size, bounds.size - 1
    length = np.zeros(n, U64) if length is None else np.asarray(length, U64)
    cap = np.full(n, cap1, U64) if cap is None else np.asarray(cap, U64)
    nlpos = np.flatnonzero(buf == 10).astype(U64)

    def before(p):  # newlines before each position
        return np.searchsorted(nlpos, p, side="left").astype(U64)

    first = np.searchsorted(start, bounds, side="left").astype(U64)
    seg = np.searchsorted(bounds, start, side="right").astype(np.int64) - 1
    ok = (seg >= 0) & (seg < nseg)
    sg = np.where(ok, seg, 0)
    rel = np.where(ok, start - bounds[sg], 0).astype(U64)
    line = np.where(ok, U64(1) + before(start) - before(bounds[sg]), 0).astype(U64)
    out = {"first": first, "rel": rel, "line": line,
           "newlines": before(bounds[1:]) - before(bounds[:-1])}
    digest, dcap, mlines = np.zeros(nseg, U64), np.zeros(nseg, U64), np.zeros(nseg, U64)
    with np.errstate(over="ignore"):
        for s in range(nseg):
            m = ok & (seg == s)
            digest[s] = (rel[m] * U64(31) + length[m]).sum(dtype=U64)
            dcap[s] = ((rel[m] + U64(1)) * cap[m]).sum(dtype=U64)
            mlines[s] = np.unique(line[m]).size
    out.update(digest=digest, dcap=dcap, mlines=mlines)
    return out


def _cases(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def fixture_tables():
    """The fixture tables of the seam property: (set name, label, opc, word)
    for every table of anchor_cases, wordb_cases, lookahead_cases, redo_cases
    (without option N), word_cases under option W, asgroup_cases (compiled
    here) and patterns.json, once each."""
    import ugrep_amd as U
    out, seen = [], set()

    def add(setname, label, opc, word=False):
        key = (tuple(int(x) for x in opc), word)
        if key not in seen:
            seen.add(key)
            out.append((setname, label, list(key[0]), word))

    for name in ("anchor_cases", "wordb_cases", "lookahead_cases", "redo_cases"):
        for c in _cases(name)["cases"]:
            if not c.get("nul"):
                add(name, c["pattern"], c["opc"])
    for c in _cases("word_cases"):
        add("word_cases", c["pattern"], c["opc"], word=True)
    for c in _cases("asgroup_cases")["cases"]:
        try:
            add("asgroup_cases", c["pattern"], U.compile_regex(c["pattern"]))
        except U.Unsupported:
            pass  # (the compiler refuses it: tests/test_asgroup.py REFUSED)
    for k, p in _cases("patterns").items():
        add("patterns", k, p["opc"])
    return out


def oracle_find(o, data, word=False):
    """The oracle's record list of `data` ([start, len, cap] rows)."""
    return (o.find_w(data, want_list=True) if word else o.find(data, want_list=True))[3]


def per_input_lists(o, inputs, word=False):
    """The per-input record lists shifted to packed offsets, concatenated."""
    _, bounds = pack(inputs)
    rows = []
    for d, b in zip(inputs, bounds[:-1]):
        rows += [[s + int(b), ln, cp] for s, ln, cp in oracle_find(o, np.frombuffer(bytes(d), np.uint8), word)]
    return rows


def random_inputs(rng, k, maxlen=40, endings=ENDINGS):
    """k short inputs over an alphabet that meets the fixture patterns, each
    with one of the endings (the first is empty)."""
    alpha = np.frombuffer(b"foobarbaz FOO _-.,;\n\n\r\n\t09(){}=x\xc3\xa9\xe2\x82\xac", np.uint8)
    out = [b""]
    for i in range(1, k):
        body = alpha[rng.integers(0, alpha.size, int(rng.integers(0, maxlen)))].tobytes()
        if i % 3 == 0:
            body = b"foo" + body + b"foo"
        d = body + endings[int(rng.integers(0, len(endings)))]
        if d.endswith(b"\r") and BARE_CR not in endings:
            d += b"\n"  # (the body's own '\r' must not make a bare-CR ending)
        out.append(d)
    return out


__all__ = ["pack", "split", "fixture_tables", "oracle_find", "per_input_lists", "random_inputs", "ENDINGS",
           "BARE_CR"]
