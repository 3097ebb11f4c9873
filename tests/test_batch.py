"""GPU: batched FIND (ugpu_find_batch) and its device split
(ugpu_split_matches).  The split is compared with the numpy model
(tests/batch_model.py, checked by hand in tests/test_batch_host.py) on
synthetic sorted lists; find_batch is compared, input by input and record by
record, with find_all over each input alone, the oracle restatement and numpy
line counts."""
import json
import os

import numpy as np
import pytest

import batch_model as bm
from oracle_lib import GOLDEN, REPO, OracleDfa, gen

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A5A5A5A5A
U64 = np.uint64


@pytest.fixture(scope="module")
def U():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


def _golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


# ---------------------------------------------------------------- ugpu_split_matches
def _dev_u8(data):
    import torch
    buf = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    if len(data):
        buf[:len(data)].copy_(torch.from_numpy(np.array(data, dtype=np.uint8)))
    return buf


def _dev_arr(a, dt):
    import torch
    a = np.ascontiguousarray(np.asarray(a, dtype=dt))
    if not a.size:
        return None
    return torch.from_numpy(a.view(np.int64 if dt == np.uint64 else np.int32).copy()).to("cuda")


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _split(U, buf, n, bounds, start, length, cap, cap1=0, rel=True, line=True):
    """ugpu_split_matches through device arrays with canaries behind them;
    returns the model's dict layout."""
    import torch
    nseg, m = len(bounds) - 1, len(start)
    db, ds = _dev_arr(bounds, np.uint64), _dev_arr(start, np.uint64)
    dl = None if length is None else _dev_arr(length, np.uint32)
    dc = None if cap is None else _dev_arr(cap, np.uint32)
    seg = torch.full((5, nseg + 2), CANARY, dtype=torch.int64, device="cuda")
    rec = torch.full((2, m + 1), CANARY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    U.split_matches(buf.data_ptr(), n, db.data_ptr(), nseg, _ptr(ds), _ptr(dl), _ptr(dc), cap1, m,
                    seg[0].data_ptr(), seg[1].data_ptr(), seg[2].data_ptr(), seg[3].data_ptr(), seg[4].data_ptr(),
                    rec[0].data_ptr() if rel else 0, rec[1].data_ptr() if line else 0)
    torch.cuda.synchronize()
    s = seg.cpu().numpy().view(np.uint64)
    r = rec.cpu().numpy().view(np.uint64)
    assert s[0, nseg + 1] == CANARY and (s[1:, nseg:] == CANARY).all()
    assert (r[:, m:] == CANARY).all()
    if not rel:
        assert (r[0] == CANARY).all()
    if not line:
        assert (r[1] == CANARY).all()
    return {"first": s[0, :nseg + 1], "digest": s[1, :nseg], "dcap": s[2, :nseg], "newlines": s[3, :nseg],
            "mlines": s[4, :nseg], "rel": r[0, :m] if rel else None, "line": r[1, :m] if line else None}


def _check_split(U, data, bounds, start, length, cap, cap1=0, rel=True, line=True, buf=None, what=""):
    want = bm.split(data, bounds, start, length, cap, cap1)
    got = _split(U, _dev_u8(data) if buf is None else buf, len(data), bounds, start, length, cap, cap1, rel, line)
    for k in ("first", "digest", "dcap", "newlines", "mlines", "rel", "line"):
        if got[k] is not None:
            assert np.array_equal(got[k], want[k]), (what, k)
    return got


def _text(n, seed, line=40):
    """n bytes of letters with a newline about every `line` bytes."""
    rng = np.random.default_rng(seed)
    a = rng.integers(97, 123, n).astype(np.uint8)
    a[rng.random(n) < 1.0 / line] = 10
    return a


def _records(rng, n, m):
    """m distinct sorted starts below n with lengths and accept indices."""
    start = np.sort(rng.choice(n, size=m, replace=False)).astype(U64)
    return start, rng.integers(0, 9, m).astype(np.uint32), rng.integers(1, 5, m).astype(np.uint32)


def test_split_small_shapes(U):
    n = 100000 + 3
    data = _text(n, 1)
    buf = _dev_u8(data)
    rng = np.random.default_rng(2)
    st, ln, cp = _records(rng, n, 3000)
    # no record
    _check_split(U, data, [0, 10, 5000, n], [], [], [], buf=buf, what="n=0")
    # one segment: the whole buffer, an inner range
    _check_split(U, data, [0, n], st, ln, cp, buf=buf, what="nseg=1")
    _check_split(U, data, [777, 90001], st, ln, cp, buf=buf, what="nseg=1 inner")
    # a wave of 64 records over 4 segments, records exactly at the bounds
    w = np.arange(64, dtype=U64) * U64(7) + U64(100)
    _check_split(U, data, [100, 100 + 7 * 10, 100 + 7 * 30, 100 + 7 * 31, 100 + 7 * 64], w, ln[:64], cp[:64], buf=buf,
                 what="wave over 4 segments")
    # runs of empty segments at the start, in the middle and at the end
    _check_split(U, data, [0, 0, 0, 5000, 5000, 5000, 5000, 90000, n, n, n], st, ln, cp, buf=buf, what="empty runs")
    _check_split(U, data, [4096, 4096, 8192, 8192, 8192], st, ln, cp, buf=buf, what="empty runs, tile bounds")
    # a segment over several waves and blocks between two small ones; records at every bound
    b = [int(st[5]), int(st[40]), int(st[2500]), int(st[2600])]
    _check_split(U, data, b, st, ln, cp, buf=buf, what="long segment")
    # records outside [bounds[0], bounds[nseg])
    got = _check_split(U, data, [int(st[100]) + 1, 50000, int(st[-50])], st, ln, cp, buf=buf, what="outside")
    assert int(got["first"][0]) == 101 and int(got["first"][-1]) == 3000 - 50
    assert not got["rel"][:101].any() and not got["line"][-50:].any()
    # optional arrays
    _check_split(U, data, [0, 30000, n], st, ln, None, cap1=3, buf=buf, what="cap NULL")
    _check_split(U, data, [0, 30000, n], st, None, cp, buf=buf, what="len NULL")
    _check_split(U, data, [0, 30000, n], st, None, None, cap1=3, rel=False, buf=buf, what="rel NULL")
    _check_split(U, data, [0, 30000, n], st, ln, cp, line=False, buf=buf, what="line NULL")
    _check_split(U, data, [0, 30000, n], st, ln, cp, rel=False, line=False, buf=buf, what="both NULL")


def test_split_lines_across_waves_and_blocks(U):
    """Lines of 20 bytes; two records on one line sit at the record indices
    63 | 64 (a wave boundary) and 255 | 256 (a block boundary): mlines counts
    the line once.  The other records are on consecutive lines."""
    nlines = 600
    data = np.full(20 * nlines, ord("x"), np.uint8)
    data[19::20] = 10
    start, line = [], 0
    for i in range(520):
        if i in (64, 256, 300):
            start.append(start[-1] + 5)  # the previous record's line
        else:
            start.append(20 * line + (i % 19))
            line += 1
    start = np.asarray(start, U64)
    for bounds in ([0, len(data)], [0, 20 * 64, 20 * 200, len(data)], [20 * 63, 20 * 63 + 5, 20 * 254, len(data)]):
        got = _check_split(U, data, bounds, start, None, None, cap1=1, what=str(bounds))
    whole = _check_split(U, data, [0, len(data)], start, None, None, cap1=1)
    assert int(whole["mlines"][0]) == 517 and int(whole["newlines"][0]) == nlines
    # a record on the newline itself belongs to the line that newline ends
    _check_split(U, data, [0, 40, len(data)], [19, 20, 39, 40, 59], None, None, cap1=2, what="on newlines")


def test_split_4mib(U):
    """A buffer of 4 MiB - 37 bytes (every wave range of the walk), 3000
    segments with repeats, the last bound at len, 200000 records."""
    n = (4 << 20) - 37
    data = _text(n, 3, line=60)
    rng = np.random.default_rng(4)
    st, ln, cp = _records(rng, n, 200000)
    bounds = np.sort(rng.choice(n, size=3000, replace=True)).astype(U64)
    bounds[-1] = n
    bounds[100:110] = bounds[100]
    bounds = np.sort(bounds)
    _check_split(U, data, bounds, st, ln, cp, what="4 MiB")
    # a buffer without a newline, and one that ends in the middle of a granule
    flat = np.full(70001, ord("a"), np.uint8)
    s2, l2, c2 = _records(rng, flat.size, 500)
    _check_split(U, flat, [0, 1, 70001], s2, l2, c2, what="no newline")


def test_split_repeats_exactly(U):
    n = 300000
    data = _text(n, 5)
    buf = _dev_u8(data)
    st, ln, cp = _records(np.random.default_rng(6), n, 50000)
    a = _split(U, buf, n, [0, 1000, n], st, ln, cp)
    b = _split(U, buf, n, [0, 1000, n], st, ln, cp)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- ugpu_find_batch
_INPUTS = {}


def _inputs():
    """About 300 inputs of 0 to 2 KiB cut from the generated corpora with the
    adversarial endings, two of about 300 KiB, and several empty ones in a row."""
    if "std" not in _INPUTS:
        rng = np.random.default_rng(11)
        corp = [gen(k, 3, 0, 1 << 20).tobytes() for k in (1, 2, 3, 4)]
        out = []
        for i in range(300):
            c = corp[i % 4]
            ln = int(rng.integers(0, 2048))
            off = int(rng.integers(0, len(c) - ln))
            d = c[off:off + ln]
            if i % 5 == 0:
                d = b"foo" + d + b" foobar foo"
            d += bm.ENDINGS[int(rng.integers(0, len(bm.ENDINGS)))]
            if d.endswith(b"\r"):
                d += b"\n"
            out.append(d)
            if i in (7, 150):
                out += [b"", b"", b""]
            if i == 100:
                out.append(corp[0][5000:5000 + 300 * 1024 + 13] + b"foo")
            if i == 200:
                out.append(corp[2][:300 * 1024 - 5] + b"\n")
        out += [b"", b""]
        _INPUTS["std"] = out
    return _INPUTS["std"]


def _tables():
    cfg = json.load(open(os.path.join(REPO, "ugrep_amd", "data", "config_patterns.json")))
    look = next(c for c in _golden("lookahead_cases")["cases"] if c["pattern"] == "foo(?=bar)")
    return {
        "c2": (cfg["c2_foobarbaz"]["opc"], False),
        "c3": (cfg["c3_ident"]["opc"], False),
        "c4": (cfg["c4_word"]["opc"], False),
        "w_foo": (next(c for c in _golden("word_cases") if c["pattern"] == "foo")["opc"], True),
        "bol": ("^foo", False),
        "eol": ("foo$", False),
        "wordb": (next(c for c in _golden("wordb_cases")["cases"] if c["pattern"] == "\\bfoo\\b")["opc"], False),
        "lookahead": (look["opc"], False),
        "redo": (_golden("redo_cases")["cases"][0]["opc"], False),
    }


def _line_numbers(d, starts):
    nl = np.flatnonzero(np.frombuffer(d, np.uint8) == 10)
    return 1 + np.searchsorted(nl, np.asarray(starts, np.int64), side="left"), nl.size


def _check_batch(U, pat, res, inputs, oracle=None, find_all=True):
    """Every input of `res` against find_all over it alone, the oracle's list
    and numpy line numbers."""
    assert len(res) == len(inputs) and int(res.first[0]) == 0 and int(res.first[-1]) == res.count
    total = 0
    for i, d in enumerate(inputs):
        fr, line = res.input(i)
        total += fr.count
        got = (fr.count, fr.digest, fr.dcap)
        if find_all:
            one = U.find_all(pat, d, offsets=True)
            assert got == (one.count, one.digest, one.dcap), i
            assert fr.triples() == one.triples(), i
        if oracle is not None:
            cnt, dg, dc, lst = oracle(np.frombuffer(d, np.uint8))
            assert got == (cnt, dg, dc), i
            assert fr.triples() == lst, i
        ln, newlines = _line_numbers(d, fr.start)
        assert int(res.newlines[i]) == newlines, i
        assert np.array_equal(line.astype(np.int64), ln), i
        assert int(res.matching_lines[i]) == np.unique(ln).size, i
    assert total == res.count


@pytest.mark.parametrize("name", ["c2", "c3", "c4", "w_foo", "bol", "eol", "wordb", "lookahead", "redo"])
def test_find_batch_one_scan(U, name):
    opc, word = _tables()[name]
    pat = U.Pattern(opc, word=word)
    o = OracleDfa(pat.opc)
    inputs = _inputs()
    res = U.find_batch(pat, inputs)
    assert res.one_scan is True
    assert res.count > 20
    _check_batch(U, pat, res, inputs, oracle=lambda b: (o.find_w if word else o.find)(b, want_list=True))


def _equal(a, b):
    assert a.count == b.count
    for k in ("first", "digest", "dcap", "newlines", "matching_lines", "start", "length", "cap", "line"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or np.array_equal(x, y), k


def test_find_batch_per_input_path(U, patterns):
    inputs = _inputs()[:60] + [b"a\n\nfoo\n\n", b"x", b""]
    # a table whose matches can contain '\n'
    opc = patterns["hello_wnhS"]["opc"]
    assert U.host_newline(opc)
    pat = U.Pattern(opc)
    res = U.find_batch(pat, inputs)
    assert res.one_scan is False and res.count > 0
    o = OracleDfa(opc)
    _check_batch(U, pat, res, inputs, oracle=lambda b: o.find(b, want_list=True))
    # option N
    pat = U.Pattern("foo", empty=True)
    res = U.find_batch(pat, inputs)
    assert res.one_scan is False and res.count > 0
    o2 = OracleDfa(pat.opc)
    _check_batch(U, pat, res, inputs, oracle=lambda b: o2.find(b, want_list=True, nul=True))


def test_find_batch_bare_cr(U):
    inputs = [b"foo\nfoo", b"x foo\r", b"", b"foo\r\nfoo\r\n", b"foo"]
    eol = U.Pattern("foo$")
    assert eol.info()["contexts"] != 1
    res = U.find_batch(eol, inputs)
    assert res.one_scan is False
    _check_batch(U, eol, res, inputs)
    assert res.input(1)[0].count == 0  # the "foo\r" tail is not matched
    assert [res.input(i)[0].count for i in range(5)] == [2, 0, 0, 2, 1]
    # without the bare CR the same table takes one scan
    assert U.find_batch(eol, [inputs[0]] + inputs[2:]).one_scan is True
    # a plain table reads no context: one scan with the bare CR too
    foo = U.Pattern("foo")
    assert foo.info()["contexts"] == 1
    res = U.find_batch(foo, inputs)
    assert res.one_scan is True
    _check_batch(U, foo, res, inputs)
    assert res.input(1)[0].count == 1


@pytest.mark.parametrize("name", ["c2", "c4", "eol"])
def test_find_batch_sub_batches(U, monkeypatch, name):
    opc, word = _tables()[name]
    pat = U.Pattern(opc, word=word)
    inputs = _inputs()[:130]  # (holds one input of 300 KiB)
    assert max(len(d) for d in inputs) > 4096
    whole = U.find_batch(pat, inputs)
    monkeypatch.setenv("UGPU_BATCH_BYTES", "4096")
    cut = U.find_batch(pat, inputs)
    assert cut.one_scan is True and whole.one_scan is True
    _equal(whole, cut)
    # COUNT mode: no record arrays, the same per-input totals
    cnt = U.find_batch(pat, inputs, offsets=False)
    assert cnt.start is None and cnt.line is None and cnt.count == whole.count
    for k in ("first", "digest", "dcap", "newlines", "matching_lines"):
        assert np.array_equal(getattr(cnt, k), getattr(whole, k)), k


def test_find_batch_edge_calls(U):
    pat = U.Pattern("foo")
    res = U.find_batch(pat, [])
    assert len(res) == 0 and res.count == 0 and res.first.tolist() == [0] and res.one_scan is True
    res = U.find_batch(pat, [b"", b"", b""])
    assert res.count == 0 and res.first.tolist() == [0, 0, 0, 0]
    assert not res.newlines.any() and not res.matching_lines.any() and not res.digest.any()
    assert res.input(1)[0].count == 0 and res.input(1)[1].size == 0
    inputs = [b"", b"foo\nbar foo", b"", b"\n\nfoo"]
    cnt = U.find_batch(pat, inputs, offsets=False)
    full = U.find_batch(pat, inputs)
    assert cnt.start is None and cnt.length is None and cnt.cap is None and cnt.line is None
    assert cnt.count == full.count == 3
    assert np.array_equal(cnt.digest, full.digest) and np.array_equal(cnt.dcap, full.dcap)
    assert cnt.input(1)[0].count == 2 and cnt.input(1)[1] is None
    assert full.line.tolist() == [1, 2, 3] and full.start.tolist() == [0, 8, 2]
    assert full.newlines.tolist() == [0, 1, 0, 2] and full.matching_lines.tolist() == [0, 2, 0, 1]
    # a NULL input with a length
    import ctypes
    L = U._lib
    ptrs = (ctypes.c_void_p * 2)(None, None)
    lens = (ctypes.c_uint64 * 2)(0, 5)
    out = ctypes.POINTER(L.BatchResult)()
    assert L.lib.ugpu_find_batch(pat.handle, ptrs, lens, 2, L.MODE_OFFSETS, ctypes.byref(out)) == L.UGPU_INVAL
    assert not out
    # numpy and host-tensor inputs
    import torch
    mixed = [np.frombuffer(b"foo\n", np.uint8), torch.from_numpy(np.frombuffer(b"a foo", np.uint8).copy()), b"foo"]
    res = U.find_batch(pat, mixed)
    assert res.first.tolist() == [0, 1, 2, 3] and res.start.tolist() == [0, 2, 0]
