"""Host side of the n-gram kernel (kernel 7): the plan, the filter's superset
property and selectivity, and the golden cases through the oracle restatement.
No GPU needed."""
import json
import os

import numpy as np
import pytest

import ugrep_amd
import wordset_gen
from oracle_lib import OracleDfa, gen as host_gen

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_NGRAM = 64
SIZES = (100, 300, 1000, 3000)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "wordset_cases.json")) as f:
        return json.load(f)["cases"]


_OPC = {}


def set_opc(n, **kw):
    key = (n, tuple(sorted(kw.items())))
    if key not in _OPC:
        _OPC[key] = ugrep_amd.compile_regex(wordset_gen.regex(wordset_gen.words(n)), **kw)
    return _OPC[key]


@pytest.fixture
def no_ng_env(monkeypatch):
    monkeypatch.delenv("UGPU_NG", raising=False)


@pytest.mark.parametrize("word", (False, True))
@pytest.mark.parametrize("n", SIZES)
def test_plan_takes_ngram_kernel(n, word, no_ng_env):
    info = ugrep_amd.host_plan(set_opc(n), word=word)
    assert info["format"] in (1, 2)
    assert info["kernel"] == 7
    assert info["shape"] & SHAPE_NGRAM
    assert 0 < info["prefilter_ppm"] <= 150001
    g = ugrep_amd.host_ngram(set_opc(n), word=word)
    assert g["enabled"] and g["n"] == 4 and g["ppm"] == info["prefilter_ppm"]


def test_plan_covers_both_formats(no_ng_env):
    assert {ugrep_amd.host_plan(set_opc(n))["format"] for n in SIZES} == {1, 2}


@pytest.mark.parametrize("word", (False, True))
@pytest.mark.parametrize("n", SIZES)
def test_plan_ng0_restores(n, word, monkeypatch):
    monkeypatch.setenv("UGPU_NG", "0")
    info = ugrep_amd.host_plan(set_opc(n), word=word)
    assert info["kernel"] == (4 if info["format"] == 2 or word else 1)
    assert not info["shape"] & SHAPE_NGRAM
    assert info["prefilter_ppm"] == 0
    assert not ugrep_amd.host_ngram(set_opc(n), word=word)["enabled"]


def test_plan_unchanged_elsewhere(no_ng_env):
    # byte tables keep sparse_kernel
    info = ugrep_amd.host_plan(set_opc(30))
    assert (info["format"], info["kernel"]) == (0, 0) and not info["shape"] & SHAPE_NGRAM
    # dense first n-grams: the estimate is over the bound
    for rx, k in ((r"\w+ \w+", 4), (r"\D\D", 1)):
        info = ugrep_amd.host_plan(rx)
        assert info["kernel"] == k and not info["shape"] & SHAPE_NGRAM, rx
    # a 1-byte word: n < 2, no filter
    opc = ugrep_amd.compile_regex(wordset_gen.regex(wordset_gen.words(100) + ["q"]))
    info = ugrep_amd.host_plan(opc)
    assert info["format"] == 1 and info["kernel"] == 1 and not info["shape"] & SHAPE_NGRAM
    assert ugrep_amd.host_ngram(opc) is None
    # option N
    for n in (100, 1000):
        info = ugrep_amd.host_plan(set_opc(n), empty=True)
        assert info["kernel"] != 7 and not info["shape"] & SHAPE_NGRAM


def _texts(ws):
    out = [("edge", np.frombuffer(wordset_gen.edge_text(ws), np.uint8))]
    for kind in (1, 3, 4):
        out.append(("gen%d" % kind, wordset_gen.plant(host_gen(kind, 5, 0, 262144), ws)))
    return out


def _accepting(o, buf):
    """positions from which the oracle's walk accepts (matches have >= 2 bytes,
    so a chain step from p that ends past p + 1 is a match at p)"""
    acc = np.zeros(len(buf), bool)
    for p in range(len(buf)):
        acc[p] = o.chain_exit(buf, p, p + 1) > p + 1
    return acc


@pytest.mark.parametrize("n", (300, 1000))
def test_superset_and_selectivity(n, no_ng_env):
    ws = wordset_gen.words(n)
    opc = set_opc(n)
    g = ugrep_amd.host_ngram(opc)
    ng = g["n"]
    prefixes = {w.encode("utf-8")[:ng] for w in ws}
    o = OracleDfa(opc)
    for name, buf in _texts(ws):
        buf = np.ascontiguousarray(buf)
        flags = ugrep_amd.host_ngram_candidates(opc, buf).astype(bool)
        acc = _accepting(o, buf)
        assert acc.sum() > 0, name
        assert not (acc & ~flags).any(), (name, np.flatnonzero(acc & ~flags)[:5])
        # the last n - 1 positions cannot start a match and are not flagged
        assert not flags[len(buf) - ng + 1:].any()
        raw = buf.tobytes()
        true = sum(raw[p:p + ng] in prefixes for p in range(len(raw) - ng + 1))
        print("%s: flagged %d true prefixes %d of %d, fill %.5f" % (name, flags.sum(), true, len(raw), g["fill"]))
        assert true <= flags.sum()
        assert flags.sum() / len(raw) <= true / len(raw) + 2 * g["fill"], name


def test_candidates_short_buffers(no_ng_env):
    opc = set_opc(100)
    w = wordset_gen.words(100)[0].encode()
    for ln in range(0, 6):
        f = ugrep_amd.host_ngram_candidates(opc, w[:ln])
        assert len(f) == ln and f.sum() == (1 if ln >= 4 else 0)


def test_golden_through_oracle(golden):
    for c in golden:
        ws = wordset_gen.words(c["words"], c["seed"])
        opc = c["opc"] if c["opc"] is not None else ugrep_amd.compile_regex(wordset_gen.regex(ws), icase=c["icase"])
        o = OracleDfa(opc)
        word = c["mode"].endswith("W")
        for r in c["results"]:
            if r["input"] == "edge":
                buf = np.frombuffer(wordset_gen.edge_text(ws), np.uint8)
            else:
                _, kind, seed, off, ln = r["spec"].split(":")
                buf = host_gen(int(kind), int(seed), int(off), int(ln))
            got = o.find_w(buf, want_list=True) if word else o.find(buf, want_list=True)
            assert got[:3] == (r["count"], r["digest"], r["dcap"]), (c["name"], r["input"])
            if r["list"] is not None:
                assert got[3] == r["list"], (c["name"], r["input"])


def test_icase_native_compile_matches_reference(golden):
    c = next(c for c in golden if c["icase"])
    ws = wordset_gen.words(c["words"], c["seed"])
    o = OracleDfa(ugrep_amd.compile_regex(wordset_gen.regex(ws), icase=True))
    for r in c["results"]:
        if r["input"] == "edge":
            got = o.find(np.frombuffer(wordset_gen.edge_text(ws), np.uint8), want_list=True)
            assert got[3] == r["list"]
