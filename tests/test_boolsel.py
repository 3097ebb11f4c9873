"""GPU: Boolean line queries (ugpu_select_lines_bool, grep_bool): the lines
satisfying a CNF over several match lists, --files and -v included.  Pinned to
what the reference CLI prints for its own --bool suite
(tests/golden/boolsel_cases.json), to ugpu_select_lines for the one-list
formulas, and to the numpy model (tests/boolsel_model.py, itself pinned to the
reference by tests/test_boolsel_host.py) on edge buffers and seeded inputs."""
import json
import os

import numpy as np
import pytest

import boolsel_model as B
import linesel_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 0x5A5A5A5A5A5A5A5A
MODES = {"-n": (False, 0), "-n --files": (True, 0), "-nC2": (False, 2), "-nC2 --files": (True, 2)}
FLAGS = [(False, False), (True, False), (False, True), (True, True)]  # (invert, files)


@pytest.fixture(scope="module")
def U():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def boolsel():
    with open(os.path.join(GOLDEN, "boolsel_cases.json")) as f:
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


def _dev_lists(lists):
    """[(starts, lens or None)] -> the (d_start, d_len, n) triples and the tensors that back them."""
    import torch
    keep, out = [], []
    for starts, lens in lists:
        m = len(starts)
        st = torch.from_numpy(np.asarray(starts, dtype=np.uint64).view(np.int64).copy()).to("cuda")
        ln = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.uint32).view(np.int32).copy()).to("cuda")
        keep += [st, ln]
        out.append((st.data_ptr() if m else 0, ln.data_ptr() if ln is not None and m else 0, m))
    return out, keep


def _select(U, buf, n, dl, clauses, invert, files, slack=3):
    """(selected, lines, whole, begin, end, lineno) of one count-only call and
    one write call; the record arrays carry `slack` canaries behind the capacity."""
    import torch
    torch.cuda.synchronize()
    sel, lines, whole = U.select_lines_bool(buf.data_ptr(), n, dl, clauses, invert, files)
    rec = torch.full((3, sel + slack), CANARY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    got = U.select_lines_bool(buf.data_ptr(), n, dl, clauses, invert, files, rec[0].data_ptr(), rec[1].data_ptr(),
                              rec[2].data_ptr(), sel)
    torch.cuda.synchronize()
    assert got == (sel, lines, whole)
    r = _u64(rec)
    assert (r[:, sel:] == CANARY).all()
    return sel, lines, whole, r[0, :sel], r[1, :sel], r[2, :sel]


def _check(U, data, lists, clauses, what="", flags=FLAGS, buf=None):
    buf = _dev(data) if buf is None else buf
    dl, keep = _dev_lists(lists)
    for invert, files in flags:
        wb, we, wl, wn, ww = B.select(data, lists, clauses, invert, files)
        sel, lines, whole, b, e, ln = _select(U, buf, len(data), dl, clauses, invert, files)
        assert (sel, lines, whole) == (len(wl), wn, ww), (what, invert, files)
        assert np.array_equal(ln, wl), (what, invert, files)
        assert np.array_equal(b, wb) and np.array_equal(e, we), (what, invert, files)
    del keep


def _case_lists(c):
    out = []
    for m in c["matches"]:
        m = np.asarray(m, np.int64).reshape(-1, 2)
        out.append((m[:, 0], m[:, 1]))
    return out


# ---------------------------------------------------------------- reference goldens
def test_reference_cases_select(U, boolsel):
    for c in boolsel["cases"]:
        data = _file(c["file"])
        buf = _dev(data)
        lists = _case_lists(c)
        dl, keep = _dev_lists(lists)
        clauses = [tuple(x) for x in c["clauses"]]
        tb, te = M.line_table(data)
        for mode, files in (("-n", False), ("-n --files", True)):
            files = files and len(lists) > 0  # (no pattern: the reference's primary matches every line)
            sel, lines, whole, b, e, ln = _select(U, buf, len(data), dl, clauses, False, files)
            want = [x[0] for x in c["printed"][mode]]
            assert ln.tolist() == want and sel == len(want), (c["query"], c["file"], mode)
            assert lines == len(tb)
            assert b.tolist() == tb[ln.astype(np.int64) - 1].tolist(), (c["query"], c["file"], mode)
            assert e.tolist() == te[ln.astype(np.int64) - 1].tolist(), (c["query"], c["file"], mode)
            if files:
                assert whole == (sel > 0), (c["query"], c["file"])
        _check(U, data, lists, clauses, c["query"] + " " + c["file"], buf=buf)  # -v too, against the model


def test_reference_cases_grep_bool(U, boolsel):
    for c in boolsel["cases"]:
        data = _file(c["file"])
        lines = data.tobytes().split(b"\n")
        q = c["query"] if c["bool"] else (c["patterns"], [tuple(x) for x in c["clauses"]])
        for mode, (files, ctx) in MODES.items():
            r = U.grep_bool(q, data.tobytes(), files=files, before=ctx, after=ctx)
            got = [list(x) for x in zip(r.lineno.tolist(), r.kind.tolist())]
            assert got == c["printed"][mode], (c["query"], c["file"], mode)
            for ln, b, e in zip(r.lineno.tolist(), r.begin.tolist(), r.end.tolist()):
                assert data[b:e].tobytes() == lines[ln - 1], (c["query"], c["file"], mode, ln)


def test_grep_bool_refuses_newline_patterns(U):
    with pytest.raises(ValueError):
        U.grep_bool(r"Hello \S\n\S", b"Hello\nWorld\n")
    with pytest.raises(ValueError):
        U.grep_bool((["Hello", r"a\nb"], [(1, 0), (0, 2)]), b"Hello\nWorld\n")
    r = U.grep_bool("hello -world", b"Hello\nHello World\n", icase=True)
    assert r.lineno.tolist() == [1]
    r = U.grep_bool("hello -world", b"Hello\nHello World\n", icase=True, invert=True)
    assert r.lineno.tolist() == [2]


# ---------------------------------------------------------------- equivalence with ugpu_select_lines
def _edge_buffer():
    d = np.full(3 * 4096 + 77, ord("a"), np.uint8)
    for p in (0, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 3 * 4096 + 76):
        d[p] = 10
    return d


def test_one_list_equals_select_lines(U):
    import torch
    d = _edge_buffer()
    n = len(d)
    buf = _dev(d)
    rng = np.random.default_rng(5)
    cases = [(np.zeros(0, np.int64), None), (np.arange(0, n, 7), np.ones(len(np.arange(0, n, 7)), np.uint32))]
    for nst in (1, 7, 300):
        starts = np.sort(rng.choice(n, size=nst, replace=False))
        cases += [(starts, None), (starts, rng.integers(0, 40, nst).astype(np.uint32)),
                  (starts, rng.integers(0, 6000, nst).astype(np.uint32))]
    cases.append((np.array([n // 2, n - 1, n, n + 1, n + 5000], np.uint64), np.array([1, 1, 1, 0, 3], np.uint32)))
    for starts, lens in cases:
        dl, keep = _dev_lists([(starts, lens)])
        for invert in (False, True):
            torch.cuda.synchronize()
            sel, lines = U.select_lines(buf.data_ptr(), n, dl[0][0], dl[0][1], dl[0][2], invert)
            rec = torch.zeros((3, max(sel, 1)), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            U.select_lines(buf.data_ptr(), n, dl[0][0], dl[0][1], dl[0][2], invert, rec[0].data_ptr(),
                           rec[1].data_ptr(), rec[2].data_ptr(), sel)
            want = _u64(rec)[:, :sel]
            # {pos=1} is select_lines, {neg=1} is select_lines with UGPU_SEL_INVERT; -v swaps them
            for clause, inv in (((0, 1) if invert else (1, 0), False), ((1, 0) if invert else (0, 1), True)):
                s2, l2, _, b, e, ln = _select(U, buf, n, dl, [clause], inv, False)
                assert (s2, l2) == (sel, lines), (len(starts), invert, clause)
                assert np.array_equal(np.stack([b, e, ln]), want), (len(starts), invert, clause)


# ---------------------------------------------------------------- carries and crowds
def _long_line():
    d = np.full(3 * 4096 + 77 + 40, ord("x"), np.uint8)
    d[10] = 10                       # line 1
    d[10 + 3 * 4096 + 77 + 1] = 10   # line 2: 3 * 4096 + 77 bytes
    d[-1] = 10                       # line 3
    return d


def test_long_line_literals_from_different_tiles(U):
    """One line over three tiles; list 0 matches in tile 0, list 1 in tile 2,
    list 2 on line 3 only: the literals of the long line are decided where it
    ends, from the covers carried across the waves."""
    d = _long_line()
    a = 11  # begin of the long line
    lists = [([a + 5], [3]), ([a + 2 * 4096 + 300], [2]), ([len(d) - 5], [1])]
    buf = _dev(d)
    dl, keep = _dev_lists(lists)
    sel, lines, _, b, e, ln = _select(U, buf, len(d), dl, [(1, 0), (2, 0)], False, False)
    assert (sel, lines, b.tolist(), e.tolist(), ln.tolist()) == (1, 3, [a], [a + 3 * 4096 + 77], [2])
    for clauses in ([(1, 0), (2, 0)], [(1, 0), (0, 2)], [(0, 1), (2, 0)], [(3, 0), (0, 4)], [(4, 3)], [(0, 3)],
                    [(1, 0), (2, 0), (0, 4)], [(4, 0)], [(5, 0), (6, 0)]):
        _check(U, d, lists, clauses, "long line %r" % (clauses,), buf=buf)
    # a match of list 1 that starts in tile 0 and reaches line 3; one on the long line's newline
    _check(U, d, [([a + 5], [3]), ([a + 100], [3 * 4096 + 10])], [(1, 0), (2, 0)], "reaching", buf=buf)
    _check(U, d, [([a + 5], [3]), ([a + 3 * 4096 + 77], [1])], [(1, 0), (2, 0)], "on its newline", buf=buf)
    _check(U, d, [([a + 5], [3]), ([a + 3 * 4096 + 77], [2])], [(0, 1), (2, 0)], "newline and next line", buf=buf)


def test_cover_carried_across_ranges(U):
    """Matches of two lists reaching over newline-bearing tiles without a
    match of their own (a range is one tile at this size)."""
    d = np.full(5 * 4096 + 3, ord("b"), np.uint8)
    d[np.arange(50, len(d), 300)] = 10
    s, last = 100, 3 * 4096 + 500
    lists = [([s], [last - s + 1]), ([4096 + 10, 4 * 4096 + 1000], [2 * 4096, 0]), ([20, s + 4096], [1, 1])]
    for clauses in ([(1, 0), (2, 0)], [(1, 0), (0, 2)], [(2, 1), (4, 0)], [(0, 1), (0, 2), (0, 4)], [(7, 0)]):
        _check(U, d, lists, clauses, "carried %r" % (clauses,))


def test_many_matches_one_tile(U):
    """More than 64 matches of one list in one tile (several steps of the
    match loop), beside a sparse list."""
    d = np.full(9000, ord("c"), np.uint8)
    d[[99, 4999, 8999]] = 10
    d[np.arange(300, 1200, 50)] = 10
    crowd = np.arange(200, 200 + 300 * 3, 3)
    lists = [(crowd, np.ones(300, np.uint32)), ([150, 5000], [2, 1]), (crowd[::2] + 1, None)]
    for clauses in ([(1, 0)], [(1, 0), (0, 2)], [(4, 0), (2, 1)], [(0, 4), (1, 0)]):
        _check(U, d, lists, clauses, "crowd %r" % (clauses,))


def test_sixteen_lists_sixty_four_clauses(U):
    rng = np.random.default_rng(17)
    n = 2 * 4096 + 321
    d = np.where(rng.random(n) < 0.05, 10, 100).astype(np.uint8)
    lists = []
    for t in range(16):
        st = np.sort(rng.choice(n, size=int(rng.integers(1, 400)), replace=False))
        lists.append((st, rng.integers(0, 30, len(st)).astype(np.uint32)))
    lists[3] = (np.zeros(0, np.int64), None)   # an empty list, used negated and plain below
    lists[9] = (np.zeros(0, np.int64), np.zeros(0, np.uint32))
    clauses = []
    for c in range(64):
        pos = int(rng.integers(0, 1 << 16)) & int(rng.integers(0, 1 << 16))
        neg = int(rng.integers(0, 1 << 16)) & int(rng.integers(0, 1 << 16)) & int(rng.integers(0, 1 << 16))
        clauses.append((pos | 1 << (c % 16), neg))
    clauses[0] = (1 << 3 | 1 << 5, 0)       # the empty list in a pos mask
    clauses[1] = (0, 1 << 3)                # and alone in a neg mask: always true
    clauses[2] = (1 << 9, 1 << 2)
    _check(U, d, lists, clauses, "16 x 64")
    _check(U, d, lists, [(1 << 3, 0)], "only the empty list")          # nothing; -v everything
    _check(U, d, lists, [(0, 1 << 9)], "only the empty list negated")
    _check(U, d, lists, [(1 << 15, 1 << 14), (1 << 4, 0)], "high lists only")  # 3 of 16 lists used
    _check(U, d, lists, [], "no clause")


def test_unterminated_empty_and_emptyline(U):
    d = np.frombuffer(b"one foo\ntwo bar\nlast foo bar", np.uint8)
    lists = [([4, 21], [3, 3]), ([12, 25], [3, 3])]
    for clauses in ([(1, 0), (2, 0)], [(1, 0), (0, 2)], [(0, 1)], [(3, 0)], []):
        _check(U, d, lists, clauses, "unterminated %r" % (clauses,))
    buf = _dev(d)
    dl, keep = _dev_lists(lists)
    sel, lines, whole, b, e, ln = _select(U, buf, len(d), dl, [(1, 0), (2, 0)], False, False)
    assert (sel, lines, b.tolist(), e.tolist(), ln.tolist()) == (1, 3, [16], [len(d)], [3])
    for name, nlines in (("empty.txt", 0), ("emptyline.txt", 1)):
        data = _file(name)
        assert M.line_table(data)[0].size == nlines
        for ls in ([], [([], None)], [([0], [0]), ([0, 1, 7], [1, 1, 2])]):
            k = len(ls)
            for clauses in ([], [(1, 0)][:k], [(0, 1)][:k], [(1, 0), (0, 2)] if k > 1 else []):
                _check(U, data, ls, clauses, name)


# ---------------------------------------------------------------- seeded inputs against the model
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_buffers(U, seed):
    rng = np.random.default_rng(seed)
    for rnd in range(6):
        n = int(rng.integers(1, 64 << 10))
        p_nl = float(rng.choice([0.0005, 0.01, 0.1, 0.5]))
        d = np.where(rng.random(n) < p_nl, 10, 120).astype(np.uint8)
        if rnd % 2:
            d[-1] = 10
        k = int(rng.integers(1, 17))
        lists = []
        for t in range(k):
            m = int(rng.choice([0, 1, 5, 100, 2000]))
            st = np.sort(rng.choice(n + 3, size=min(m, n), replace=False))  # a few at and past len
            hi = int(rng.choice([1, 4, 50, 9000]))                          # up to matches over many newlines
            lists.append((st, None if t % 5 == 4 else rng.integers(0, hi, len(st)).astype(np.uint32)))
        clauses = []
        for c in range(int(rng.integers(0, 9))):
            pos = int(rng.integers(0, 1 << k)) & int(rng.integers(0, 1 << k))
            neg = int(rng.integers(0, 1 << k)) & int(rng.integers(0, 1 << k))
            if not pos | neg:
                pos = 1 << int(rng.integers(0, k))
            clauses.append((pos, neg))
        _check(U, d, lists, clauses, "seed %d round %d" % (seed, rnd))


def test_many_waves(U):
    """64 MiB + 123 bytes (several tiles per wave range), 4 lists with clusters
    of > 64 starts in one tile, runs of empty ranges and matches longer than a
    wave range; count-only and write."""
    rng = np.random.default_rng(11)
    n = (64 << 20) + 123
    d = np.where(rng.random(n) < 0.02, 10, 97).astype(np.uint8)
    lists = []
    for t in range(4):
        parts = [np.arange(5000 + 50 * t, 5300), np.arange((t + 1) << 20, ((t + 1) << 20) + 4096, 3),
                 rng.choice(n, 2000, replace=False), np.array([t, 4095 + t, n - 1 - t])]
        st = np.unique(np.concatenate(parts)).astype(np.int64)
        ln = rng.integers(0, 200, len(st)).astype(np.uint32)
        ln[t::97] = 70000
        lists.append((st, ln))
    _check(U, d, lists, [(1, 2), (4, 0), (3, 8)], "64 MiB", flags=[(False, False)])


# ---------------------------------------------------------------- the workspace the line calls share
def test_shared_workspace_changing_slots(U):
    """The one-list call, the 16-list call and line_spans take their per-wave
    arrays from one pooled workspace: 4, 19 and 1 arrays per wave, over 4, 257
    and 1 wave ranges in turn (it grows, then is reused smaller); lines runs
    between them from its own."""
    import torch
    rng = np.random.default_rng(23)
    for n in (3 * 4096 + 5, (1 << 20) + 7, 100):
        d = np.where(rng.random(n) < 0.04, 10, 101).astype(np.uint8)
        buf = _dev(d)
        lists = []
        for t in range(16):
            st = np.sort(rng.choice(n, size=min(n, int(rng.integers(1, 200))), replace=False))
            lists.append((st, rng.integers(0, 60, len(st)).astype(np.uint32)))
        dl, keep = _dev_lists(lists)
        # select_lines with one list
        starts, lens = lists[0]
        wb, we, wl, wn = M.select(d, starts, lens, False)
        torch.cuda.synchronize()
        sel, lines = U.select_lines(buf.data_ptr(), n, dl[0][0], dl[0][1], dl[0][2], False)
        rec = torch.full((3, sel + 3), CANARY, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert U.select_lines(buf.data_ptr(), n, dl[0][0], dl[0][1], dl[0][2], False, rec[0].data_ptr(),
                              rec[1].data_ptr(), rec[2].data_ptr(), sel) == (sel, lines)
        torch.cuda.synchronize()
        r = _u64(rec)
        assert (sel, lines) == (len(wl), wn), n
        assert (r[:, sel:] == CANARY).all()
        assert np.array_equal(r[0, :sel], wb) and np.array_equal(r[1, :sel], we) and np.array_equal(r[2, :sel], wl), n
        # select_lines_bool over 16 lists, one clause naming all of them
        _check(U, d, lists, [(0x5555, 0xaaaa), (1, 0)], "shared workspace, %d bytes" % n, flags=[(False, False)],
               buf=buf)
        # line_spans for every line
        nlines = M.line_table(d)[0].size
        q = np.arange(1, nlines + 1, dtype=np.uint64)
        qd = torch.from_numpy(q.view(np.int64).copy()).to("cuda")
        out = torch.full((2, len(q) + 2), CANARY, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        U.line_spans(buf.data_ptr(), n, qd.data_ptr(), len(q), out[0].data_ptr(), out[1].data_ptr())
        torch.cuda.synchronize()
        r = _u64(out)
        sb, se = M.spans(d, q)
        assert (r[:, len(q):] == CANARY).all()
        assert np.array_equal(r[0, :len(q)], sb) and np.array_equal(r[1, :len(q)], se), n
        # lines
        ln = torch.zeros(len(starts), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        nl, ml = U.lines(buf.data_ptr(), n, dl[0][0], len(starts), ln.data_ptr())
        torch.cuda.synchronize()
        nlpos = np.flatnonzero(d == 10)
        want = 1 + np.searchsorted(nlpos, np.asarray(starts, dtype=np.int64), side="left")
        assert (nl, ml) == (len(nlpos), len(np.unique(want))), n
        assert np.array_equal(ln.cpu().numpy(), want), n
        del keep


# ---------------------------------------------------------------- capacity and arguments
def test_capacity_and_invalid_arguments(U):
    import torch
    from ugrep_amd import _lib
    d = _edge_buffer()
    n = len(d)
    buf = _dev(d)
    lists = [(np.arange(0, n, 5), None), (np.arange(3, n, 11), None)]
    dl, keep = _dev_lists(lists)
    clauses = [(3, 0)]
    wb, we, wl, wn, _ = B.select(d, lists, clauses)
    sel = len(wl)
    assert sel > 2
    torch.cuda.synchronize()
    assert U.select_lines_bool(buf.data_ptr(), n, dl, clauses)[:2] == (sel, wn)   # count only
    rec = torch.full((3, sel + 2), CANARY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(U.UgpuError) as ei:
        U.select_lines_bool(buf.data_ptr(), n, dl, clauses, False, False, rec[0].data_ptr(), rec[1].data_ptr(),
                            rec[2].data_ptr(), sel - 1)
    torch.cuda.synchronize()
    assert ei.value.code == _lib.UGPU_CAPACITY and ei.value.selected == sel and ei.value.lines == wn
    assert (_u64(rec) == CANARY).all()

    def inval(*a, **kw):
        with pytest.raises(U.UgpuError) as ei:
            U.select_lines_bool(*a, **kw)
        assert ei.value.code == _lib.UGPU_INVAL

    inval(buf.data_ptr(), n, dl, [(4, 0)])                   # a list >= nlists
    inval(buf.data_ptr(), n, dl, [(1, 0), (0, 4)])
    inval(buf.data_ptr(), n, dl, [(1, 0), (0, 0)])           # an empty clause
    inval(buf.data_ptr(), n, dl * 9, [(1, 0)])               # 18 lists
    inval(buf.data_ptr(), n, dl, [(1, 0)] * 65)              # 65 clauses
    inval(buf.data_ptr() + 1, n - 1, dl, clauses)            # alignment
    inval(buf.data_ptr(), n, [(0, 0, 5)], [(1, 0)])          # a NULL list with matches
    inval(buf.data_ptr(), n, dl, clauses, d_begin=rec[0].data_ptr(), capacity=sel)  # one record array only
    rc = _lib.lib.ugpu_select_lines_bool(buf.data_ptr(), n, None, None, None, 0, None, 0, 4, None, None, None, 0,
                                         None, None, None, None)                     # an unknown flag
    assert rc == _lib.UGPU_INVAL
    assert (_u64(rec) == CANARY).all()
