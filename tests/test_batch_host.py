"""Batched FIND, the host half (CPU): ugpu_batch_plan_host, the seam property
on the oracle that lets one scan of the packed inputs serve a whole batch, the
bare-CR exception, and the numpy model of ugpu_split_matches the GPU tests
compare against (tests/batch_model.py)."""
import collections
import json
import os

import numpy as np

import batch_model as bm
from oracle_lib import REPO, OracleDfa


def _config():
    with open(os.path.join(REPO, "ugrep_amd", "data", "config_patterns.json")) as f:
        return json.load(f)


def test_batch_plan_config_tables():
    import ugrep_amd as U
    cfg = _config()
    for k in ("c2_foobarbaz", "c3_ident", "c4_word"):
        assert U.host_batch_plan(cfg[k]["opc"]) is True, k
        assert U.host_batch_plan(cfg[k]["opc"], empty=True) is False, k
    assert U.host_batch_plan("foo$") is True
    assert U.host_batch_plan("foo$", empty=True) is False


def test_batch_plan_follows_newline(patterns):
    import ugrep_amd as U
    for k, p in patterns.items():
        for empty in (False, True):
            assert U.host_batch_plan(p["opc"], empty=empty) == (not U.host_newline(p["opc"]) and not empty), k
    newline, refused = [], 0
    for setname, label, opc, word in bm.fixture_tables():
        if not OracleDfa(opc).supported:  # (an assertion between consumed bytes: the engine refuses it too)
            refused += 1
            continue
        if U.host_newline(opc):
            newline.append(label)
            assert U.host_batch_plan(opc, word=word) is False, label
    assert len(newline) == 2 and refused == 3, (newline, refused)


def test_seam_property_on_the_oracle():
    """For every fixture table without a newline edge, FIND over the packed
    inputs equals the per-input lists shifted to packed offsets."""
    import ugrep_amd as U
    rng = np.random.default_rng(20261020)
    compared = collections.Counter()
    for setname, label, opc, word in bm.fixture_tables():
        o = OracleDfa(opc)
        if not o.supported or U.host_newline(opc):
            continue
        assert U.host_batch_plan(opc, word=word) is True, label
        for _ in range(6):
            inputs = bm.random_inputs(rng, 12)
            assert not any(d.endswith(bm.BARE_CR) for d in inputs)
            packed, _b = bm.pack(inputs)
            assert bm.oracle_find(o, packed, word) == bm.per_input_lists(o, inputs, word), (setname, label, inputs)
        compared[setname] += 1
    # nothing skipped silently: 235 distinct tables, 3 the oracle refuses, 2 with a newline edge
    assert sum(compared.values()) == 230, compared
    assert compared["word_cases"] >= 15 and compared["anchor_cases"] >= 40 and compared["wordb_cases"] >= 90
    assert compared["lookahead_cases"] >= 12 and compared["redo_cases"] >= 12 and compared["asgroup_cases"] >= 20


def test_seam_endings_are_all_drawn():
    rng = np.random.default_rng(1)
    ends = collections.Counter()
    for _ in range(50):
        for d in bm.random_inputs(rng, 12):
            ends[max((e for e in bm.ENDINGS if d.endswith(e)), key=len)] += 1
    assert all(ends[e] > 0 for e in bm.ENDINGS), ends


def test_bare_cr_is_an_exception():
    """at_eol is 0 for '\\r' then EOF but 1 for "\\r\\n": foo$ does not match
    the tail of b"foo\\r" alone and does once the separator follows."""
    import ugrep_amd as U
    o = OracleDfa(U.compile_regex("foo$"))
    alone = bm.oracle_find(o, np.frombuffer(b"foo\r", np.uint8))
    packed = bm.oracle_find(o, bm.pack([b"foo\r"])[0])
    assert alone == [] and packed == [[0, 3, 1]]
    # a plain table sees no difference
    p = OracleDfa(U.compile_regex("foo"))
    assert bm.oracle_find(p, np.frombuffer(b"foo\r", np.uint8)) == bm.oracle_find(p, bm.pack([b"foo\r"])[0])


def test_pack():
    buf, bounds = bm.pack([b"ab", b"", b"c\n", b"", b"d\r"])
    assert buf.tobytes() == b"ab\nc\nd\r\n"
    assert bounds.tolist() == [0, 3, 3, 5, 5, 8]


def test_split_model_by_hand():
    #        0123 4567 8 9
    buf = b"ab\nc" b"d\n\ne" b"\n" b"x"
    bounds = [1, 4, 4, 9]  # segments [1,4) [4,4) [4,9); bytes 0 and 9 lie outside
    start = [0, 1, 3, 4, 5, 7, 8, 9]
    length = [1, 1, 1, 1, 0, 1, 0, 1]
    cap = [1, 2, 1, 1, 3, 1, 1, 7]
    r = bm.split(np.frombuffer(buf, np.uint8), bounds, start, length, cap)
    assert r["first"].tolist() == [1, 3, 3, 7]
    assert r["rel"].tolist() == [0, 0, 2, 0, 1, 3, 4, 0]
    # segment 0 "b\nc": lines 1, 2; segment 2 "d\n\ne\n": d 1, its '\n' 1, e 3, its '\n' 3
    assert r["line"].tolist() == [0, 1, 2, 1, 1, 3, 3, 0]
    assert r["newlines"].tolist() == [1, 0, 3]
    assert r["mlines"].tolist() == [2, 0, 2]
    assert r["digest"].tolist() == [0 * 31 + 1 + 2 * 31 + 1, 0, 1 + 31 + 3 * 31 + 1 + 4 * 31]
    assert r["dcap"].tolist() == [1 * 2 + 3 * 1, 0, 1 * 1 + 2 * 3 + 4 * 1 + 5 * 1]
    # cap NULL with cap1, len NULL
    r = bm.split(np.frombuffer(buf, np.uint8), bounds, start, None, None, cap1=3)
    assert r["digest"].tolist() == [2 * 31, 0, (1 + 3 + 4) * 31]
    assert r["dcap"].tolist() == [3 * (1 + 3), 0, 3 * (1 + 2 + 4 + 5)]
