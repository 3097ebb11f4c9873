"""GPU: large string sets on the n-gram kernel (kernel 7, ngram_kernel.hip):
class and wide tables behind the hashed n-gram candidate filter.  Record by
record against the reference's golden results (tests/golden/wordset_cases.json)
and the oracle restatement: buffer lengths and starts around the n-gram and
tile sizes, words planted at the buffer end and across every tile edge (also
with wave ranges ending inside the buffer), overlapping and prefix words, long
runs of candidates, random bytes (hash collisions), streams, shards, the
records path, chain_fix, and the same results with UGPU_NG=0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wordset_gen
from wordset_child import triples_hash

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
NG = 4  # the n-gram length of these sets (words have 4 bytes or more)


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    os.environ.pop("UGPU_NG", None)
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "wordset_cases.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def set300(U):
    """(words, opc, oracle, plain pattern, W pattern) of the 300-word set"""
    from oracle_lib import OracleDfa
    ws = wordset_gen.words(300)
    opc = U.compile_regex(wordset_gen.regex(ws))
    return ws, opc, OracleDfa(opc), U.Pattern(opc), U.Pattern(opc, word=True)


@pytest.fixture(scope="module")
def corpus1m(set300):
    """1 MiB of the word corpus with words of the set planted (never modified)"""
    from oracle_lib import gen
    buf = wordset_gen.plant(gen(1, 5, 0, 1 << 20), set300[0])
    buf.setflags(write=False)
    return buf


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(r, want, what):
    """totals, and the records when the scan wrote them and the oracle listed them"""
    assert (r.count, r.digest, r.dcap) == tuple(want[:3]), what
    if want[3] is not None and r.start is not None and len(r.start) == r.count:
        assert r.triples() == want[3], what


def test_kernel_id_and_golden(U, golden):
    from oracle_lib import OracleDfa, gen
    for c in golden:
        ws = wordset_gen.words(c["words"], c["seed"])
        opc = c["opc"] if c["opc"] is not None else U.compile_regex(wordset_gen.regex(ws), icase=c["icase"])
        word = c["mode"].endswith("W")
        pat = U.Pattern(opc, word=word)
        assert pat.info()["kernel"] == 7, c["name"]
        assert pat.info()["shape"] & 64, c["name"]
        o = OracleDfa(opc)
        for r in c["results"]:
            if r["input"] == "edge":
                buf = np.frombuffer(wordset_gen.edge_text(ws), np.uint8)
            else:
                _, kind, seed, off, ln = r["spec"].split(":")
                buf = gen(int(kind), int(seed), int(off), int(ln))
            want = o.find_w(buf, want_list=True) if word else o.find(buf, want_list=True)
            assert want[:3] == (r["count"], r["digest"], r["dcap"]), (c["name"], r["input"], "oracle")
            if r["list"] is not None:
                assert want[3] == r["list"]
            dev = torch.from_numpy(np.array(buf, copy=True)).cuda()
            _same(U.find_all(pat, dev, offsets=False), want, (c["name"], r["input"], "count"))
            _same(U.find_all(pat, dev, offsets=True), want, (c["name"], r["input"], "offsets"))


def test_buffer_lengths(U, set300):
    ws, opc, o, pat, patw = set300
    base = wordset_gen.plant(np.full(3 * 4096 + 5, 32, np.uint8), ws, every=61)
    for ln in (0, 1, NG - 1, NG, NG + 1, 4095, 4096, 4097, 3 * 4096 + 5):
        # (a word at the start, and the text up to the length under test)
        buf = base[:ln].copy()
        w = np.frombuffer(ws[0].encode(), np.uint8)
        buf[:min(ln, len(w))] = w[:ln]
        if ln == 0:
            r = U.find_all(pat, b"", offsets=True)
            assert r.count == 0
            continue
        _same(U.find_all(pat, buf.tobytes(), offsets=True), o.find(buf, want_list=True), ("plain", ln))
        _same(U.find_all(patw, buf.tobytes(), offsets=True), o.find_w(buf, want_list=True), ("word", ln))


def test_starts(U, set300):
    ws, opc, o, pat, patw = set300
    from oracle_lib import gen
    buf = wordset_gen.plant(gen(1, 6, 0, 256 << 10), ws, every=499)
    dev = torch.from_numpy(buf).cuda()
    for start in (1, 99999):
        _same(U.find_all(pat, dev, start=start, offsets=True), o.find(buf, start=start, want_list=True), start)
        _same(U.find_all(patw, dev, start=start, offsets=True), o.find_w(buf, start=start, want_list=True), start)


def test_planted_at_tile_edges_and_buffer_end(U, set300):
    ws, opc, o, pat, patw = set300
    for name, buf in wordset_gen.tile_edge_buffers(ws, NG):
        want = o.find(buf, want_list=True)
        # every tile edge holds the start of a match in the d bytes before it
        d = int(name[-1])
        starts = {t[0] for t in want[3]}
        assert all(t * 4096 - d in starts for t in range(2, 16, 2)), name
        _same(U.find_all(pat, buf.tobytes(), offsets=True), want, name)
        _same(U.find_all(pat, buf.tobytes(), offsets=False), want, name)
        _same(U.find_all(patw, buf.tobytes(), offsets=True), o.find_w(buf, want_list=True), (name, "word"))
    last = dict(wordset_gen.tile_edge_buffers(ws, NG))["edge_d%d" % (NG + 1)]
    want = o.find(last, want_list=True)[3]
    assert want[-1][0] + want[-1][1] == len(last)  # a word ends at the last byte


def _child(which, env):
    e = dict(os.environ)
    e.pop("UGPU_NG", None)
    e.pop("UGPU_MAX_GRID", None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "wordset_child.py"), which], env=e, capture_output=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout.decode().strip().split("\n")[-1])


def _check_child(got, inputs, o):
    for name, buf in inputs:
        for mode, want in (("plain", o.find(buf, want_list=True)), ("word", o.find_w(buf, want_list=True))):
            assert got[name][mode] == [want[0], want[1], want[2], triples_hash(want[3])], (name, mode)


@pytest.mark.parametrize("grid", ("1", "3"))
def test_planted_at_tile_edges_small_grids(U, set300, grid):
    """wave ranges of several tiles that end inside the buffer (a fresh process:
    the grid is fixed when a scanner is created)"""
    got = _child("edges", {"UGPU_MAX_GRID": grid})
    assert got["kernel"] == {"plain": 7, "word": 7}
    _check_child(got, wordset_gen.child_inputs("edges")[1], set300[2])


def test_same_results_with_ng0(U, set300):
    got = _child("corpus", {"UGPU_NG": "0"})
    assert 7 not in got["kernel"].values()
    inputs = wordset_gen.child_inputs("corpus")[1]
    _check_child(got, inputs, set300[2])
    for name, buf in inputs:  # and this process, on kernel 7, says the same
        r = U.find_all(set300[3], buf.tobytes(), offsets=True)
        assert got[name]["plain"] == [r.count, r.digest, r.dcap, triples_hash(r.triples())], name


@pytest.fixture(scope="module")
def overlap_set(U):
    from oracle_lib import OracleDfa
    ws = ["abca", "cabc", "foo", "foobar", "barfoo"] + wordset_gen.words(80, utf8=False)
    opc = U.compile_regex(wordset_gen.regex(ws))
    pat = U.Pattern(opc)
    assert pat.info()["states"] > 256 and pat.info()["kernel"] == 7
    return opc, OracleDfa(opc), pat, U.Pattern(opc, word=True)


def test_overlaps_and_prefixes(U, overlap_set):
    opc, o, pat, patw = overlap_set
    for text in (b"abc" * 3000, b"foobar" * 1500, b"foofoobar", b"xfoobarfoo foo fo foobarfoobar barfoofoo",
                 b"cabcabca abcabc" * 700):
        buf = np.frombuffer(text, np.uint8)
        _same(U.find_all(pat, text, offsets=True), o.find(buf, want_list=True), text[:12])
        _same(U.find_all(pat, text, offsets=False), o.find(buf), text[:12])
        _same(U.find_all(patw, text, offsets=True), o.find_w(buf, want_list=True), (text[:12], "word"))


def test_long_runs(U):
    from oracle_lib import OracleDfa
    ws = ["aaaa", "aaaab"] + wordset_gen.words(80, utf8=False)
    opc = U.compile_regex(wordset_gen.regex(ws))
    pat = U.Pattern(opc)
    assert pat.info()["kernel"] == 7
    o = OracleDfa(opc)
    for tail in (b"", b"b", b"aab"):
        buf = np.frombuffer(b"a" * (1 << 20) + tail, np.uint8)
        want = o.find(buf, want_list=True)
        assert want[0] >= (1 << 18)
        _same(U.find_all(pat, buf.tobytes(), offsets=False), want, tail)
        _same(U.find_all(pat, buf.tobytes(), offsets=True), want, tail)


def test_random_bytes(U, set300):
    ws, opc, o, pat, patw = set300
    rng = np.random.default_rng(20261020)
    buf = wordset_gen.plant(rng.integers(0, 256, 1 << 20, dtype=np.uint8), ws, every=4999)
    flags = U.host_ngram_candidates(opc, buf)
    want = o.find(buf, want_list=True)
    assert flags.sum() > 4 * want[0]  # most candidates are hash collisions: their walks fail
    _same(U.find_all(pat, buf.tobytes(), offsets=True), want, "plain")
    _same(U.find_all(patw, buf.tobytes(), offsets=True), o.find_w(buf, want_list=True), "word")


def test_stream_shards_records(U, set300, corpus1m):
    ws, opc, o, pat, patw = set300
    data = corpus1m
    rng = np.random.default_rng(9)
    cuts = sorted(set(int(x) for x in rng.integers(1, data.size, 20))) + [data.size]
    for p, want in ((pat, o.find(data, want_list=True)), (patw, o.find_w(data, want_list=True))):
        assert want[0] > 100
        st = U.Stream(p, keep=4096)
        trip, i = [], 0
        for c in cuts:
            trip += st.feed(data[i:c].tobytes(), final=c == data.size).triples()
            i = c
        assert trip == want[3], "stream"
        assert U.find_all_multi(p, data, ndev=5, offsets=True).triples() == want[3], "multi"
        assert U.Records(p, data).triples() == want[3], "records"


def test_scanner_chain_fix_inside_a_word(U, set300, corpus1m):
    ws, opc, o, pat, patw = set300
    data = corpus1m
    n = data.size
    t = torch.from_numpy(np.array(data, copy=True)).cuda()
    torch.cuda.synchronize()
    whole = o.find(data, want_list=True)
    # a cut inside a match: the second shard's chain enters at the match end
    m = whole[3][len(whole[3]) // 2]
    cut = m[0] + 2
    assert cut < m[0] + m[1]
    a, b = U.Scanner(pat), U.Scanner(pat)
    a.scan(t.data_ptr(), 0, cut, n, True, 0, _stream())
    ta = a.totals()
    b.scan(t.data_ptr(), cut, n, n, True, 0, _stream())
    tb = b.totals()
    assert ta.exit == m[0] + m[1]
    d = b.chain_fix(t.data_ptr(), cut, n, n, True, 0, cut, ta.exit, _stream())
    M = 1 << 64
    got = ((ta.count + tb.count + d.count) % M, (ta.digest + tb.digest + d.digest) % M,
           (ta.dcap + tb.dcap + d.dcap) % M)
    assert got == whole[:3]
