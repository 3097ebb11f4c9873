"""CPU: the hash finite automaton (ugpu_hfa_create, hfa.cpp) and its host
evaluator (ugpu_hfa_match_host) against the reference CLI's recorded index
query (tests/golden/hfa_cases.json, made by make_hfa_golden.py) and the plain
Python restatement tests/hfa_model.py, on stores from tests/index_model.py.
Every comparison is exact."""
import json
import os

import numpy as np
import pytest

import hfa_model as H
import index_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ACCURACIES = (0, 4, 9)


@pytest.fixture(scope="module")
def U():
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "hfa_cases.json")) as f:
        g = json.load(f)
    assert g["corpus"] == H.corpus() and g["patterns"] == H.patterns()
    files = [(c["name"], H.corpus_bytes(c)) for c in g["corpus"]]
    g["names"] = [nm for nm, _ in files]
    g["records"] = {acc: [M.index_record(d, acc)[:2] for _, d in files] for acc in ACCURACIES}
    with open(os.path.join(HERE, "golden", "hfa_diverge.json")) as f:
        g["diverge"] = json.load(f)["patterns"]
    return g


@pytest.fixture(scope="module")
def queries(U, golden):
    """Per pattern (IndexQuery, the model's Flat or None without an automaton)."""
    out = []
    for p in golden["patterns"]:
        q = U.IndexQuery(p["pattern"], fixed="-F" in p["args"], icase="-i" in p["args"])
        w = q.words()
        out.append((q, H.Flat(w) if len(w) else None))
    return out


@pytest.fixture(scope="module")
def decisions(golden, queries):
    """{(pattern index, accuracy): [keep per file]} by the host evaluator, computed once."""
    out = {}
    for pi, (q, _) in enumerate(queries):
        for acc in ACCURACIES:
            out[pi, acc] = [q.keep_host(h, t) for h, t in golden["records"][acc]]
    return out


def test_fixture_pins_both_sides(golden):
    assert len(golden["patterns"]) >= 28 and len(golden["rows"]) == 3 * len(golden["patterns"])
    kept = sum(len(r["kept"]) for r in golden["rows"])
    total = len(golden["rows"]) * len(golden["names"])
    assert 5 * kept >= total and 5 * (total - kept) >= total


def test_no_matching_file_is_skipped(golden, decisions):
    for r in golden["rows"]:
        keep = decisions[r["pattern"], r["accuracy"]]
        kept = {nm for nm, k in zip(golden["names"], keep) if k}
        assert set(r["match"]) <= kept, (golden["patterns"][r["pattern"]], r["accuracy"], set(r["match"]) - kept)


def test_host_evaluator_equals_the_model(golden, queries, decisions):
    for pi, (q, flat) in enumerate(queries):
        for acc in ACCURACIES:
            model = [H.keep_record(flat if flat is not None else [], h, t) for h, t in golden["records"][acc]]
            assert model == decisions[pi, acc], (golden["patterns"][pi], acc)


def test_kept_sets_equal_the_reference(golden, decisions):
    pats = golden["patterns"]
    div = golden["diverge"]
    assert 10 * len(div) <= len(pats), "at most one in ten patterns may be listed"
    for key, why in div.items():
        assert key in {p["pattern"] for p in pats} and why.strip()
        assert any(c in key for c in "[]()*+?.\\{}^$"), "no plain literal or alternation of literals may be listed"
    for r in golden["rows"]:
        p = pats[r["pattern"]]
        if p["pattern"] in div:
            continue
        keep = decisions[r["pattern"], r["accuracy"]]
        kept = sorted(nm for nm, k in zip(golden["names"], keep) if k)
        assert kept == sorted(r["kept"]), (p, r["accuracy"])


def test_index_off_rows_have_no_automaton(golden, queries):
    for r in golden["rows"]:
        assert bool(r.get("index_off")) == (not queries[r["pattern"]][0].info["has_hfa"]), golden["patterns"][r["pattern"]]


# ---- hand-written automata: the behaviours of match_hfa as written

def table_with(hashes_by_bit, size=128):
    """A table of 0xff with bit k clear at the given hashes."""
    t = np.full(size, 0xFF, np.uint8)
    for k, hs in hashes_by_bit.items():
        for h in hs:
            t[h & (size - 1)] &= 0xFF ^ (1 << k)
    return t


def both(U, levels, table):
    w = H.pack(levels)
    a = H.match(w, table)
    b = U.IndexQuery(words=w).match_host(table)
    assert a == b
    return a


def test_first_offset_alone_propagates(U):
    # level 1: state 2's offset 0 (bit 1) passes, offset 1 (bit 0) fails; state 3 passes both, so the
    # level goes on; state 2 still marked its successor 4, which level 2 finds visited and dead
    levels = [
        [(1, False, [[(10, 10)]], [2, 3])],
        [(2, False, [[(20, 20)], [(21, 21)]], [4]), (3, False, [[(30, 30)], [(31, 31)]], [5])],
        [(4, True, [[(40, 40)], [(41, 41)], [(42, 42)]], []), (5, True, [[(50, 50)], [(51, 51)], [(52, 52)]], [])],
    ]
    t = table_with({0: [10, 31, 42], 1: [20, 30, 41], 2: [40]})
    assert both(U, levels, t) is True        # through state 4 alone (state 5's hashes are absent)
    t2 = table_with({0: [10, 31, 42], 1: [30, 41], 2: [40]})
    assert both(U, levels, t2) is False      # without state 2's first offset nothing reaches state 4


def test_dead_state_keeps_on_its_first_offset(U):
    levels = [
        [(1, False, [[(10, 10)]], [2])],
        [(2, True, [[(20, 20)], [(21, 21)]], [])],
    ]
    assert both(U, levels, table_with({0: [10], 1: [20]})) is True    # offset 1 (bit 0 at 21) would fail
    assert both(U, levels, table_with({0: [10, 21]})) is False        # the first offset fails


def test_stale_visit_bit_two_levels_later(U):
    # level 0 marks states 2 and 3 in the set level 1 reads.  Level 3 reads the same bitset, never cleared:
    # state 2's entry on level 3 is tested although nothing on level 2 led to it
    levels = [
        [(1, False, [[(10, 10)]], [2, 3])],
        [(2, False, [[(99, 99)], [(99, 99)]], [6]), (3, False, [[(30, 30)], [(31, 31)]], [7])],
        [(7, False, [[(70, 70)], [(71, 71)], [(72, 72)]], [8])],
        [(2, True, [[(60, 60)], [(61, 61)], [(62, 62)], [(63, 63)]], []),
         (8, True, [[(80, 80)], [(81, 81)], [(82, 82)], [(83, 83)]], [])],
    ]
    t = table_with({0: [10, 31, 72], 1: [30, 71], 2: [70], 3: [60]})
    assert both(U, levels, t) is True        # state 2 fails on level 1; its stale bit accepts on level 3
    assert both(U, levels, table_with({0: [10, 31, 72], 1: [30, 71], 2: [70]})) is False


def test_level_without_a_full_pass_skips(U):
    # level 1: the only state passes its first offset (successor marked) and fails the second: skip
    levels = [
        [(1, False, [[(10, 10)]], [2])],
        [(2, False, [[(20, 20)], [(21, 21)]], [3])],
        [(3, True, [[(40, 40)], [(41, 41)], [(42, 42)]], [])],
    ]
    assert both(U, levels, table_with({0: [10, 42], 1: [20, 41], 2: [40]})) is False
    assert both(U, levels, table_with({0: [10, 21, 42], 1: [20, 41], 2: [40]})) is True


def test_ranges_wrap_and_cover_the_table(U):
    # a range longer than the table meets every slot; a range that wraps past 65535 is stored as two
    levels = [[(1, True, [[(200, 200 + 127)]], [])]]
    for slot in (0, 5, 127):
        assert both(U, levels, table_with({0: [slot]})) is True
    assert both(U, levels, table_with({1: [3]})) is False
    levels = [[(1, True, [[(0, 2), (65530, 65535)]], [])]]
    assert both(U, levels, table_with({0: [65533]}, 65536)) is True
    assert both(U, levels, table_with({0: [1]}, 65536)) is True
    assert both(U, levels, table_with({0: [3, 65529]}, 65536)) is False
    q = U.IndexQuery("[^a-z ]{2}")       # a wide class: its second-level sets wrap
    w = H.Flat(q.words())
    assert int(w.lo.min()) == 0 and int(w.hi.max()) == 65535


def test_host_record_query_and_header_rules(U, golden):
    recs = golden["records"][4] + [(0, b""), (0x80, b""), (0x20 | 7, bytes([0xFF]) * 128), (0x87, bytes(128)),
                                   (0x20, b""), (0xC0, b"")]
    store = [(b"", 4, h, t) for h, t in recs]
    for pat in ("kernel", "a*"):
        q = U.IndexQuery(pat)
        for kw in ({}, {"ignore_binary": True}, {"decompress": True}, {"ignore_binary": True, "decompress": True}):
            got = q.query(store, device=False, **kw)     # ugpu_hfa_query_host, the fallback without a device
            assert list(got) == [q.keep_host(h, t, **kw) for h, t in recs], (pat, kw)
            assert list(got) == [H.keep_record(q.words(), h, t, **kw) for h, t in recs], (pat, kw)
            if pat == "a*":
                assert got.all()                          # no automaton: the index is off, headers included
    q = U.IndexQuery("kernel")
    assert list(q.query(store, device=False)[-6:]) == [False, True, False, q.match_host(bytes(128)), False, False]
    assert list(q.query(store, device=False, ignore_binary=True)[-6:]) == [False] * 6


def test_flags_and_info(U):
    assert U.lib.ugpu_abi_version() == 3
    q = U.IndexQuery("a*")
    assert q.info["has_hfa"] == 0 and len(q.words()) == 0 and q.match_host(bytes([0xFF]) * 128)
    with pytest.raises(U.Unsupported):
        U.IndexQuery("a+?b")
    i = U.IndexQuery("kernel").info
    assert (i["has_hfa"], i["levels"], i["truncated"]) == (1, 5, 0)   # cut at "kerne": its edge leads to the accept
    assert U.IndexQuery("ab|abcd").info["levels"] == 1                 # the first edge of "a" leads to "ab", which accepts
    assert U.IndexQuery("kernel", icase=True).info["hashes"] > i["hashes"]
    assert U.IndexQuery("a(bc)*d", fixed=True).info["levels"] == 6
    with pytest.raises(U.UgpuError):
        U.IndexQuery(words=np.array([H.MAGIC, 1, 1, 1, 1, 0, 2, 0], np.uint32))   # cut short
    bad = H.pack([[(1, True, [[(5, 5)]], [])]])
    bad[-1] = 9 | (3 << 16)                                            # lo > hi
    with pytest.raises(U.UgpuError):
        U.IndexQuery(words=bad)
