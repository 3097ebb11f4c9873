"""GPU: line records (ugpu_select_lines, ugpu_line_spans; SURVEY.md §8f row 2,
the bol/eol half): the lines a match list touches, the untouched ones (-v),
context lines and their byte spans.  Pinned to the reference's recorded CLI
outputs (tests/golden/linesel_cases.json) and to the numpy model
(tests/linesel_model.py, itself pinned to those outputs by
tests/test_linesel_host.py) on edge buffers and seeded corpora."""
import json
import os

import numpy as np
import pytest

import linesel_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FULL = 0xFFFFFFFFFFFFFFFF
CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def U():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def linesel():
    with open(os.path.join(GOLDEN, "linesel_cases.json")) as f:
        return json.load(f)


def _file(name):
    return np.frombuffer(open(os.path.join(GOLDEN, "verify", name), "rb").read(), np.uint8)


def _dev(data):
    import torch
    n = len(data)
    buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    if n:
        buf[:n].copy_(torch.from_numpy(np.array(data, dtype=np.uint8)))  # (a writable copy)
    return buf


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _select(U, buf, n, starts, lens, invert, slack=3):
    """(selected, lines, begin, end, lineno) of one count-only call and one
    write call; the record arrays carry `slack` canaries behind the capacity."""
    import torch
    m = len(starts)
    st = torch.from_numpy(np.asarray(starts, dtype=np.uint64).view(np.int64).copy()).to("cuda")
    ln = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.uint32).view(np.int32).copy()).to("cuda")
    lp = ln.data_ptr() if ln is not None and m else 0
    sp = st.data_ptr() if m else 0
    torch.cuda.synchronize()
    sel, lines = U.select_lines(buf.data_ptr(), n, sp, lp, m, invert)
    rec = torch.full((3, sel + slack), CANARY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    got = U.select_lines(buf.data_ptr(), n, sp, lp, m, invert, rec[0].data_ptr(), rec[1].data_ptr(),
                         rec[2].data_ptr(), sel)
    torch.cuda.synchronize()
    assert got == (sel, lines)
    r = _u64(rec)
    assert (r[:, sel:] == CANARY).all()
    return sel, lines, r[0, :sel], r[1, :sel], r[2, :sel]


def _check(U, data, starts, lens, what=""):
    buf = _dev(data)
    for invert in (False, True):
        wb, we, wl, wn = M.select(data, starts, lens, invert)
        sel, lines, b, e, ln = _select(U, buf, len(data), starts, lens, invert)
        assert (sel, lines) == (len(wl), wn), (what, invert)
        assert np.array_equal(ln, wl), (what, invert)
        assert np.array_equal(b, wb) and np.array_equal(e, we), (what, invert)


def _spans(U, buf, n, lineno):
    import torch
    q = torch.from_numpy(np.asarray(lineno, dtype=np.uint64).view(np.int64).copy()).to("cuda")
    out = torch.full((2, len(lineno) + 2), CANARY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    U.line_spans(buf.data_ptr(), n, q.data_ptr(), len(lineno), out[0].data_ptr(), out[1].data_ptr())
    torch.cuda.synchronize()
    r = _u64(out)
    assert (r[:, len(lineno):] == CANARY).all()
    return r[0, :len(lineno)], r[1, :len(lineno)]


# ---------------------------------------------------------------- reference goldens
def test_reference_cases_select(U, linesel):
    for c in linesel["cases"]:
        data = _file(c["file"])
        m = np.asarray(c["matches"], np.int64).reshape(-1, 2)
        buf = _dev(data)
        for opt, invert in (("-n", False), ("-nv", True)):
            if opt not in c["printed"]:
                continue
            sel, lines, b, e, ln = _select(U, buf, len(data), m[:, 0], m[:, 1], invert)
            want = [x[0] for x in c["printed"][opt]]
            assert ln.tolist() == want and sel == len(want), (c["file"], c["pattern"], opt)
            tb, te = M.line_table(data)
            assert lines == len(tb)
            assert b.tolist() == tb[ln.astype(np.int64) - 1].tolist(), (c["file"], c["pattern"], opt)
            assert e.tolist() == te[ln.astype(np.int64) - 1].tolist(), (c["file"], c["pattern"], opt)
            if "counts" in c and not invert:
                assert sel == c["counts"]["-c"], (c["file"], c["pattern"])
            if "counts" in c and invert:
                # -cv is the newline count minus -c (src/ugrep.cpp:10625-10631): it leaves out an
                # unterminated last line that -nv prints (tests/test_linesel_host.py cv_count)
                assert int(np.count_nonzero(e < len(data))) == c["counts"]["-cv"], (c["file"], c["pattern"])


def _pattern(U, patterns, c):
    if c["patterns_key"]:
        return U.Pattern(patterns[c["patterns_key"]]["opc"])
    return U.Pattern(U.compile_regex(c["regex"]))


def test_reference_cases_grep_lines(U, linesel, patterns):
    for c in linesel["cases"]:
        if c["derived"]:
            continue
        data = _file(c["file"])
        lines = data.tobytes().split(b"\n")
        pat = _pattern(U, patterns, c)
        for opt, invert, ctx in (("-n", False, 0), ("-nv", True, 0), ("-nC2", False, 2), ("-nvC2", True, 2)):
            r = U.grep_lines(pat, data.tobytes(), invert=invert, before=ctx, after=ctx)
            got = [list(x) for x in zip(r.lineno.tolist(), r.kind.tolist())]
            assert got == c["printed"][opt], (c["file"], c["pattern"], opt)
            for ln, b, e in zip(r.lineno.tolist(), r.begin.tolist(), r.end.tolist()):
                assert data[b:e].tobytes() == lines[ln - 1], (c["file"], c["pattern"], opt, ln)


def test_reference_end_to_end_find_all(U, linesel, patterns):
    """patterns.json tables -> find_all -> select_lines, for the two patterns
    the reference's own match goldens cover (refgold.json)."""
    import torch
    for c in linesel["cases"]:
        if c["patterns_key"] not in ("hello", "hello_wnhS"):
            continue
        data = _file(c["file"])
        buf = _dev(data)
        torch.cuda.synchronize()
        r = U.find_all(U.Pattern(patterns[c["patterns_key"]]["opc"]), buf[:len(data)], offsets=True)
        assert [list(x) for x in zip(r.start.tolist(), r.length.tolist())] == c["matches"]
        for opt, invert in (("-n", False), ("-nv", True)):
            sel, lines, b, e, ln = _select(U, buf, len(data), r.start, r.length, invert)
            assert ln.tolist() == [x[0] for x in c["printed"][opt]], (c["file"], c["pattern"], opt)


def test_empty_and_emptyline(U):
    for name, nlines in (("empty.txt", 0), ("emptyline.txt", 1)):
        data = _file(name)
        assert M.line_table(data)[0].size == nlines
        _check(U, data, [], None, name)
        _check(U, data, [0], [0], name)
        _check(U, data, [0, 1, 7], [1, 1, 2], name)


# ---------------------------------------------------------------- edge buffers
def _edge_buffer():
    d = np.full(3 * 4096 + 77, ord("a"), np.uint8)
    for p in (0, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 3 * 4096 + 76):
        d[p] = 10
    d[[1, 18, 4098]] = 0x0b
    d[[14, 4094]] = 0x09
    return d


def _long_line():
    d = np.full(3 * 4096 + 77 + 40, ord("x"), np.uint8)
    d[10] = 10                       # line 1
    d[10 + 3 * 4096 + 77 + 1] = 10   # line 2: 3 * 4096 + 77 bytes
    d[-1] = 10                       # line 3
    return d


EDGE = {
    "borders": _edge_buffer,
    "borders_unterminated": lambda: _edge_buffer()[:-1],
    "ragged": lambda: _edge_buffer()[:3 * 4096 + 5],
    "only_newlines": lambda: np.full(10000, 10, np.uint8),
    "no_newline": lambda: np.frombuffer(b"no newline at all" * 500, np.uint8),
    "long_line": _long_line,
    "quarter_newlines": lambda: (np.random.default_rng(3).integers(0, 4, 40000) * 3 + 7).astype(np.uint8),
}


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_buffers(U, name):
    d = EDGE[name]()
    n = len(d)
    rng = np.random.default_rng(5)
    _check(U, d, [], None, name)                                   # nothing selected / everything inverted
    every = np.arange(0, n, 7)
    _check(U, d, every, np.ones(len(every), np.uint32), name)      # dense
    for nst in (1, 7, 300):
        starts = np.sort(rng.choice(n, size=min(n, nst), replace=False))
        _check(U, d, starts, None, name + " zero-length")
        _check(U, d, starts, rng.integers(0, 40, len(starts)).astype(np.uint32), name + " short")
        _check(U, d, starts, rng.integers(0, 6000, len(starts)).astype(np.uint32), name + " long")
    # starts at and past len are ignored
    starts = np.array([n // 2, n - 1, n, n + 1, n + 5000], np.uint64)
    _check(U, d, starts, np.array([1, 1, 1, 0, 3], np.uint32), name + " past len")
    _check(U, d, starts[2:], np.array([1, 0, 3], np.uint32), name + " only past len")


def test_long_line_begin_carried(U):
    d = _long_line()
    a = 11  # begin of the long line
    # matches only in the line's first tile, only in its last tile, on its newline
    _check(U, d, [a + 5, a + 100], [3, 1], "first tile")
    _check(U, d, [a + 3 * 4096 + 60], [2], "last tile")
    _check(U, d, [a + 3 * 4096 + 77], [1], "on its newline")
    _check(U, d, [a + 3 * 4096 + 77], [2], "newline and the next line")
    buf = _dev(d)
    sel, lines, b, e, ln = _select(U, buf, len(d), [a + 5], [1], False)
    assert (sel, lines, b.tolist(), e.tolist(), ln.tolist()) == (1, 3, [a], [a + 3 * 4096 + 77], [2])


def test_cover_carried_across_ranges(U):
    """One match from tile 0 into tile 3 over newline-bearing tiles without a
    match of their own (a range is one tile at this size)."""
    d = np.full(5 * 4096 + 3, ord("b"), np.uint8)
    d[np.arange(50, len(d), 300)] = 10
    s, last = 100, 3 * 4096 + 500
    _check(U, d, [s], [last - s + 1], "spanning match")
    _check(U, d, [s, 4 * 4096 + 1000], [last - s + 1, 0], "spanning match and a later one")
    _check(U, d, [20, s], [1, last - s + 1], "an earlier one and the spanning match")
    # a short match after the start of a long one must not shorten the cover
    _check(U, d, [s, s + 4096], [last - s + 1, 1], "nested")
    # one that ends exactly on a newline does not reach the next line
    nl = int(np.flatnonzero(d == 10)[20])
    _check(U, d, [s], [nl - s + 1], "ends on a newline")
    _check(U, d, [nl], [1], "starts on a newline")
    _check(U, d, [nl], [2], "starts on a newline, reaches the next line")


def test_many_matches_one_line(U):
    d = np.full(9000, ord("c"), np.uint8)
    d[[99, 4999, 8999]] = 10
    starts = np.arange(200, 200 + 300 * 3, 3)
    buf = _dev(d)
    sel, lines, b, e, ln = _select(U, buf, len(d), starts, np.ones(300, np.uint32), False)
    assert (sel, lines, b.tolist(), e.tolist(), ln.tolist()) == (1, 3, [100], [4999], [2])
    _check(U, d, starts, np.ones(300, np.uint32), "300 on one line")


# ---------------------------------------------------------------- capacity
def test_capacity_and_count_only(U):
    import torch
    d = _edge_buffer()
    buf = _dev(d)
    starts = np.arange(0, len(d), 5)
    st = torch.from_numpy(starts.astype(np.int64)).to("cuda")
    wb, we, wl, wn = M.select(d, starts, None)
    torch.cuda.synchronize()
    assert U.select_lines(buf.data_ptr(), len(d), st.data_ptr(), 0, len(starts)) == (len(wl), wn)  # count only
    sel = len(wl)
    assert sel > 2
    rec = torch.full((3, sel + 2), CANARY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(U.UgpuError) as ei:
        U.select_lines(buf.data_ptr(), len(d), st.data_ptr(), 0, len(starts), False, rec[0].data_ptr(),
                       rec[1].data_ptr(), rec[2].data_ptr(), sel - 1)
    torch.cuda.synchronize()
    from ugrep_amd import _lib
    assert ei.value.code == _lib.UGPU_CAPACITY and ei.value.selected == sel and ei.value.lines == wn
    assert (_u64(rec)[:, sel - 1:] == CANARY).all()
    # n = 0 inverted selects every line
    tb, te = M.line_table(d)
    s2, l2, b, e, ln = _select(U, buf, len(d), [], None, True)
    assert s2 == l2 == len(tb) and b.tolist() == tb.tolist() and e.tolist() == te.tolist()
    assert ln.tolist() == list(range(1, len(tb) + 1))


# ---------------------------------------------------------------- line_spans
@pytest.mark.parametrize("name", sorted(EDGE))
def test_line_spans_edge_buffers(U, name):
    d = EDGE[name]()
    buf = _dev(d)
    nlines = M.line_table(d)[0].size
    every = np.arange(0, nlines + 2, dtype=np.uint64)  # line 0 and line lines + 1 included
    rng = np.random.default_rng(9)
    for q in (every, np.repeat(every, 3), np.sort(rng.choice(every, size=min(len(every), 50))),
              np.array([0], np.uint64), np.array([nlines + 1, nlines + 7, FULL], np.uint64)):
        b, e = _spans(U, buf, len(d), q)
        wb, we = M.spans(d, q)
        assert np.array_equal(b, wb) and np.array_equal(e, we), (name, len(q))
    assert _spans(U, buf, len(d), [0, nlines + 1])[0].tolist() == [FULL, FULL]


def test_line_spans_64_queries_one_tile(U):
    d = (np.random.default_rng(13).integers(0, 8, 6 * 4096 + 9) + 7).astype(np.uint8)  # 1/8 newlines
    buf = _dev(d)
    nl = np.flatnonzero(d == 10)
    first = int(np.searchsorted(nl, 2 * 4096)) + 2  # lines that lie whole inside tile 2
    q = np.arange(first, first + 64, dtype=np.uint64)
    assert nl[first + 64] < 3 * 4096
    b, e = _spans(U, buf, len(d), q)
    wb, we = M.spans(d, q)
    assert np.array_equal(b, wb) and np.array_equal(e, we)
    assert _spans(U, _dev(np.zeros(0, np.uint8)), 0, [0, 1, 2])[1].tolist() == [FULL] * 3


# ---------------------------------------------------------------- corpora
@pytest.fixture(scope="module")
def corpus_c2(U, patterns):
    from oracle_lib import gen
    data = gen(1, 21, 0, 16 << 20)
    r = U.find_all(U.Pattern(patterns["c2_foobarbaz"]["opc"]), data.tobytes(), offsets=True)
    return data, r.start.copy(), r.length.copy()


def test_corpus_c2(U, corpus_c2):
    data, starts, lens = corpus_c2
    _check(U, data, starts, lens, "c2")


@pytest.mark.parametrize("pname,kind", [("c3_ident", 3), ("c4_word", 4)])
def test_corpus_lines(U, patterns, pname, kind):
    from oracle_lib import gen
    data = gen(kind, 21, 0, 16 << 20)
    r = U.find_all(U.Pattern(patterns[pname]["opc"]), data.tobytes(), offsets=True)
    _check(U, data, r.start, r.length, pname)


def test_many_waves_clusters(U):
    """64 MiB + 123 bytes (several tiles per wave range): match clusters of
    > 64 starts inside one tile, runs of empty ranges, starts on range borders."""
    rng = np.random.default_rng(11)
    n = (64 << 20) + 123
    d = np.where(rng.random(n) < 0.02, 10, 97).astype(np.uint8)
    parts = [np.arange(5000, 5300), np.arange(1 << 20, (1 << 20) + 4096, 3),
             rng.choice(n, 2000, replace=False), np.array([0, 4095, 4096, n - 1])]
    starts = np.unique(np.concatenate(parts)).astype(np.int64)
    lens = rng.integers(0, 200, len(starts)).astype(np.uint32)
    lens[::97] = 70000  # a few matches longer than a wave range
    _check(U, d, starts, lens, "64 MiB")
    # spans of a sample of its lines, first and last included
    nlines = M.line_table(d)[0].size
    q = np.unique(np.concatenate([rng.choice(nlines, 3000) + 1, [1, 2, nlines - 1, nlines]])).astype(np.uint64)
    b, e = _spans(U, _dev(d), n, q)
    wb, we = M.spans(d, q)
    assert np.array_equal(b, wb) and np.array_equal(e, we)


def test_grep_lines_corpus(U, patterns, corpus_c2):
    data, starts, lens = corpus_c2
    r = U.grep_lines(U.Pattern(patterns["c2_foobarbaz"]["opc"]), data, before=2, after=3)
    lineno, kind, begin, end = M.grep(data, starts, lens, False, 2, 3)
    assert np.array_equal(r.lineno, np.asarray(lineno, np.uint64))
    assert np.array_equal(r.kind, np.asarray(kind, np.uint8))
    assert np.array_equal(r.begin, begin.astype(np.uint64)) and np.array_equal(r.end, end.astype(np.uint64))
