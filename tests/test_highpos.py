"""GPU: scans and line consumers at byte offsets past 2^31 and 2^32.

One device buffer of 2^32 + 1 MiB bytes (tests/highpos.py): filler, and two
2 MiB windows around the seams 2^31 and 2^32 that hold a mixed corpus with
planted bytes on the seam -- matches that end at, start at and cross it, a
304 KiB run of one letter, split UTF-8 characters, line ends.  Every kernel id
(0 to 7) scans ranges of the windows, from a cursor and the whole buffer, and
every record is compared with the oracle's; the line consumers run over the
whole buffer on the oracle's match lists and are compared with the numpy
models.  Expected values are folded from one window (tests/highpos.py); the CPU
test tests/test_highpos_host.py proves the folding on a small copy of the
layout.  A position, record start, bit index or line offset cut to 32 bits
anywhere gives a wrong record here."""
import numpy as np
import pytest

import highpos as H
from oracle_lib import first_nul, gen, is_binary, oracle_dfa, utf8_first_bad

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

L = H.full_layout()
NW = len(L.seams)
LAST = NW - 1
U64 = np.uint64


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def tabs(U, patterns):
    return H.tables(U, patterns)


@pytest.fixture(scope="module")
def base():
    b = H.base_window(L)
    b.setflags(write=False)
    return b


class HighBuffer:
    """The device buffer: two torch fills, then the windows."""

    def __init__(self, base):
        self.base = base
        self.buf = torch.empty(L.N + 16, dtype=torch.uint8, device="cuda")
        self.refill()
        assert self.buf.data_ptr() % 16 == 0

    def refill(self):
        """Filler everywhere, then the base windows."""
        self.buf.fill_(H.F)
        self.buf[L.P - 1:L.N:L.P] = 10
        self.buf[L.N:] = 0
        self.set(self.base)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    @property
    def data(self):
        return self.buf[:L.N]

    def set(self, win):
        """Both windows hold `win` from here on."""
        t = torch.from_numpy(np.array(win, dtype=np.uint8)).to("cuda")   # (a copy: `base` is read-only)
        for w in range(NW):
            self.buf[L.wbase(w):L.wend(w)].copy_(t)
        torch.cuda.synchronize()

    def restore(self):
        self.set(self.base)


@pytest.fixture(scope="module")
def hb(base):
    b = HighBuffer(base)
    yield b
    del b.buf
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, U64)).view(np.int64).copy()).to("cuda")


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint32)).view(np.int32).copy()).to("cuda")


def _pattern(U, t):
    """The table's Pattern; call inside t.environ()."""
    pat = U.Pattern(t.opc, word=t.word)          # (a table the engine refuses raises here: none may)
    assert pat.info()["kernel"] == t.kernel, t.name
    return pat


def _scan(sc, hb, lo, hi, bias=0):
    """Totals and records (uint64 arrays) of Scanner range [lo, hi)."""
    sc.scan(hb.ptr, lo, hi, L.N, True, bias, _stream())
    tot = sc.totals()
    n = int(tot.count)
    s = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    ln = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    cp = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    sc.offsets(s.data_ptr(), ln.data_ptr(), cp.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    rec = (s[:n].cpu().numpy().view(U64), ln[:n].cpu().numpy().view(np.uint32).astype(U64),
           cp[:n].cpu().numpy().view(np.uint32).astype(U64))
    return (n, int(tot.digest), int(tot.dcap), int(tot.exit)), rec


def _same(got, want, what):
    assert got[0].dtype == U64 and want[0].dtype == U64
    for g, w, f in zip(got, want, ("start", "len", "cap")):
        if not np.array_equal(g, w):
            m = min(g.size, w.size)
            d = np.flatnonzero(g[:m] != w[:m])
            k = int(d[0]) if d.size else m
            raise AssertionError("%s differs from record %d on (%d records, %d expected; got %r, expected %r): %r"
                                 % (f, k, g.size, w.size, g[k:k + 3].tolist(), w[k:k + 3].tolist(), what))


def _find_result(r):
    return r.start.astype(U64), r.length.astype(U64), r.cap.astype(U64)


def test_buffer_layout(hb, base):
    """The analytic newline prefix of the last window, once, with torch."""
    for w in range(NW):
        assert int((hb.buf[:L.wbase(w)] == 10).sum()) == L.newlines_before(w, base)
        assert int(hb.buf[L.wbase(w) - 1]) == 10
        assert np.array_equal(hb.buf[L.wbase(w):L.wend(w)].cpu().numpy(), base)
    assert L.N == (1 << 32) + (1 << 20) and int(hb.buf[L.N - 1]) == 10 and int(hb.buf[L.N - 2]) == H.F


RANGE_CASES = [(ti, group, w) for ti in range(H.N_TABLES) for group in ("seam", "run")
               for w in ((0, LAST) if ti in H.BOTH else (LAST,))]


@pytest.mark.parametrize("ti,group,w", RANGE_CASES)
def test_scanner_ranges(U, tabs, hb, base, ti, group, w):
    """Scanner.scan over four ranges of window w -- below the seam, across it
    with the whole run inside, from the seam and from the byte behind it --
    with the default grid and UGPU_MAX_GRID=3, once with a bias of 2^40
    (highpos.scan_plan), for sparse tables with staged and rebuilt records:
    totals with exit, then the records one by one."""
    t = tabs[ti]
    plan = H.scan_plan(group, t)
    stages = (False, True) if t.stage else (None,)
    try:
        with t.environ():
            pat = _pattern(U, t)
            for name in (t.variants[3:4] if group == "run" else t.variants[:3] + t.variants[4:]):
                # fresh scanners for every variant: a scanner that met a UMIX lead stays on the exact U kernel
                scs = {}
                for grid in (None, 3):
                    with t.environ(**({"UGPU_MAX_GRID": grid} if grid else {})):
                        for stage in stages:
                            scs[grid, stage] = U.Scanner(pat)
                            if stage is not None:
                                scs[grid, stage].stage(stage)
                win = H.variant(L, base, name, t)
                hb.set(win)
                ranges, chains = H.scan_ranges(L, w), {}
                for ri, grid, bias in plan:
                    lo, hi = ranges[ri]
                    if ri not in chains:
                        chains[ri] = H.shift(H.records(t, win, lo - L.wbase(w)), L.wbase(w))
                    for stage in stages:
                        what = (t.name, name, w, lo, hi, grid, stage, bias)
                        with t.environ(**({"UGPU_MAX_GRID": grid} if grid else {})):
                            tot, rec = _scan(scs[grid, stage], hb, lo, hi, bias)
                        assert tot == H.totals(chains[ri], hi, bias), what
                        _same(rec, H.shift(H.head(chains[ri], hi), bias), what)
                for sc in scs.values():
                    sc.close()
    finally:
        hb.restore()


@pytest.mark.parametrize("ti", range(H.N_TABLES))
def test_find_all_from_a_cursor_and_whole_buffer(U, tabs, hb, base, ti):
    """find_all(start = the window's second byte) in OFFSETS and COUNT mode
    (the xc In bits indexed by absolute position, the record download), and
    from 0 for the tables that are dead on filler, on the cross variant; the
    other variants (the long run among them, 0.3 s and more per call on the
    forest FIND) from the last window's cursor.  A table that matches filler
    runs from the last window's cursor only: its chain from an earlier one
    passes through 2 GiB of filler, which the references do not model."""
    t = tabs[ti]
    dead = H.dead_on_filler(L, t)
    try:
        with t.environ():
            pat = _pattern(U, t)
            for name in t.variants:
                win = H.variant(L, base, name, t)
                hb.set(win)
                starts = [L.wbase(w) + 1 for w in ((0, LAST) if t.both and dead else (LAST,))] + ([0] if dead else [])
                if name != "cross":   # every cursor on one variant; the others from the last window's cursor
                    starts = starts[-2:-1] if dead else starts
                for cur in starts:
                    w = max(v for v in range(NW) if L.wbase(v) <= max(cur, L.wbase(0)))
                    want = H.folded_records(L, t, win, w, cur or None)
                    r = U.find_all(pat, hb.data, start=cur, offsets=True)
                    assert (r.count, r.digest, r.dcap) == H.totals(want, L.N)[:3], (t.name, name, cur)
                    _same(_find_result(r), want, (t.name, name, cur))
                    r = U.find_all(pat, hb.data, start=cur, offsets=False)
                    assert (r.count, r.digest, r.dcap) == H.totals(want, L.N)[:3], (t.name, name, cur, "count")
    finally:
        hb.restore()


@pytest.mark.parametrize("tname", ["c3_ident", "c4_word", "aa/dense", "a+"])
def test_shard_cuts_at_the_seam(U, tabs, hb, base, tname):
    """Two Scanner shards cut at S-1, S and S+1 plus chain_fix equal one scan
    (the arithmetic of test_gpu.test_shard_split_and_stitch), which equals the
    oracle's chain, in both windows."""
    t = {x.name: x for x in tabs}[tname]
    M = 1 << 64
    try:
        with t.environ():
            pat = _pattern(U, t)
            a, b = U.Scanner(pat), U.Scanner(pat)
            for name in ("cross", "run"):
                win = H.variant(L, base, name, t)
                hb.set(win)
                chain = H.records(t, win, 0)
                for w in range(NW):
                    lo, S, hi = L.wbase(w), L.seams[w], L.N if w == LAST else L.wend(w) - 64
                    want = H.totals(H.shift(chain, lo), hi)
                    for cut in (S - 1, S, S + 1):
                        a.scan(hb.ptr, lo, cut, L.N, True, 0, _stream())
                        ta = a.totals()
                        b.scan(hb.ptr, cut, hi, L.N, True, 0, _stream())
                        tb = b.totals()
                        cnt, dg, dc, ex = ta.count + tb.count, ta.digest + tb.digest, ta.dcap + tb.dcap, tb.exit
                        if ta.exit != cut:
                            d = b.chain_fix(hb.ptr, cut, hi, L.N, True, 0, cut, ta.exit, _stream())
                            cnt, dg, dc = cnt + d.count, dg + d.digest, dc + d.dcap
                            if d.exit != M - 1:   # (2^64 - 1: the exit stays)
                                ex = d.exit
                        assert (cnt % M, dg % M, dc % M, ex) == want, (tname, name, w, cut)
    finally:
        hb.restore()


@pytest.mark.parametrize("tname", ["c3_ident", "c2_foobarbaz"])
def test_records_from_the_window(U, tabs, hb, base, tname):
    """Records(start = the window's base): every popped record and drain()'s
    totals (the packed record formats store start - base)."""
    t = {x.name: x for x in tabs}[tname]
    try:
        with t.environ():
            pat = _pattern(U, t)
            win = H.variant(L, base, "cross", t)
            hb.set(win)
            for w in range(NW):
                want = H.folded_records(L, t, win, w, L.wbase(w))
                tot = H.totals(want, L.N)[:3]
                r = U.Records(pat, hb.data, start=L.wbase(w))
                got = np.asarray(r.triples(), dtype=U64).reshape(-1, 3)
                assert r.totals() == tot, (tname, w)
                r.close()
                assert got.shape[0] == want[0].size
                assert got.shape[0] >= (200 if tname == "c3_ident" else 1)
                for sl in (slice(0, 100), slice(-100, None), slice(None)):
                    _same((got[sl, 0], got[sl, 1], got[sl, 2]), tuple(x[sl] for x in want), (tname, w, sl))
                r = U.Records(pat, hb.data, start=L.wbase(w))
                assert r.drain() == tot, (tname, w)
                r.close()
    finally:
        hb.restore()


# --- a match of 2^32 bytes or more: its length does not fit a record --------

@pytest.fixture
def giant(U, tabs, hb, base):
    """The buffer with 'a' in [0, R), R = 2^32 + 4096, and '\\n' at R; the a+
    table, and its chain: the one match (0, R), then the oracle's records of
    the rest of the last window."""
    t = {x.name: x for x in tabs}["a+"]
    R = (1 << 32) + 4096
    rest = base[R + 1 - L.wbase(LAST):]
    cap = H.records(t, np.frombuffer(b"aa", np.uint8), 0)[2][:1]
    want = H.concat([(np.zeros(1, U64), np.asarray([R], U64), cap), H.shift(H.records(t, rest, 0), R + 1)])
    try:
        hb.buf[:R].fill_(ord("a"))
        hb.buf[R] = 10
        torch.cuda.synchronize()
        with t.environ():
            yield _pattern(U, t), want
    finally:
        hb.refill()


def test_match_of_4gib_counted_and_its_records_refused(U, hb, giant):
    """COUNT totals carry the 64-bit length; every call that would hand out the
    record with its 32-bit length returns UGPU_UNSUPPORTED instead."""
    pat, want = giant
    assert int(want[1][0]) >= 1 << 32
    sc = U.Scanner(pat)
    sc.scan(hb.ptr, 0, L.N, L.N, True, 0, _stream())
    tot = sc.totals()
    assert (tot.count, tot.digest, tot.dcap, tot.exit) == H.totals(want, L.N)
    n = int(tot.count)
    out = torch.zeros((3, n), dtype=torch.int64, device="cuda")
    with pytest.raises(U.Unsupported):
        sc.offsets(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), n, _stream())
    r = U.find_all(pat, hb.data, offsets=False)
    assert (r.count, r.digest, r.dcap) == H.totals(want, L.N)[:3]
    with pytest.raises(U.Unsupported):
        U.find_all(pat, hb.data, offsets=True)
    # from behind the run nothing is that long: the records come back
    r = U.find_all(pat, hb.data, start=int(want[1][0]), offsets=True)
    _same(_find_result(r), tuple(x[1:] for x in want), "behind the run")


# --- line consumers: the whole buffer, match lists from the oracle -----------

def _lists(tabs, win):
    by = {t.name: t for t in tabs}
    a = H.folded_records(L, by["c3_ident"], win, 0, None)
    b = H.folded_records(L, by["c2_foobarbaz"], win, 0, None)
    return [(a[0], a[1]), (b[0], b[1]), H.seam_list(L)], a


@pytest.fixture(scope="module", params=["nl", "crlf"])
def lined_host(request, tabs, base):
    """The nl / crlf variant of the window, its folded line table and the match lists."""
    win = H.variant(L, base, request.param)
    return (win, H.Lines(L, win)) + _lists(tabs, win)


@pytest.fixture
def lined(lined_host, hb):
    """That variant in the buffer's windows for one test, the lists on the device too."""
    win, lines, lists, rec = lined_host
    hb.set(win)
    dlists = [(_dev64(s), _dev32(ln)) for s, ln in lists]
    try:
        yield lines, lists, dlists, rec
    finally:
        hb.restore()


def _line_records(call, sel):
    """The records of a select call: `call(begin, end, lineno, capacity)`."""
    rec = torch.full((3, max(sel, 1)), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out = call(rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), sel)
    torch.cuda.synchronize()
    return tuple(x[:sel].cpu().numpy().view(U64) for x in rec), out


@pytest.mark.parametrize("mode", ["1", "2"])
def test_lines(U, hb, lined, mode, monkeypatch):
    """ugpu_lines with the dense and the sparse assign pass: newlines, the -c
    count and the line of every match."""
    monkeypatch.setenv("UGPU_LINES_MODE", mode)
    lines, lists, dlists, _ = lined
    for (s, _), (ds, _) in zip(lists, dlists):
        out = torch.zeros(s.size, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        nl, ml = U.lines(hb.ptr, L.N, ds.data_ptr(), s.size, out.data_ptr())
        torch.cuda.synchronize()
        wnl, wml, wline = lines.line_of(s)
        assert (nl, ml) == (wnl, wml)
        assert np.array_equal(out.cpu().numpy().view(U64), wline)


@pytest.mark.parametrize("invert", [False, True])
def test_select_lines(U, hb, lined, invert):
    lines, lists, dlists, _ = lined
    for (s, ln), (ds, dl) in zip(lists, dlists):
        want = lines.select(s, ln, invert)
        sel, nlines = U.select_lines(hb.ptr, L.N, ds.data_ptr(), dl.data_ptr(), s.size, invert)
        assert (sel, nlines) == (want[0].size, want[3])
        got, out = _line_records(lambda b, e, k, c: U.select_lines(hb.ptr, L.N, ds.data_ptr(), dl.data_ptr(), s.size,
                                                                    invert, b, e, k, c), sel)
        assert out == (sel, nlines)
        for g, w in zip(got, want[:3]):
            assert np.array_equal(g, w)


def test_line_spans(U, hb, lined):
    """Lines on both sides of each seam, the last line and one past it."""
    lines = lined[0]
    q = []
    for S in L.seams:
        k = int(lines.line_of(np.asarray([S], U64))[2][0])
        q += [k - 1, k, k + 1, k + 2]
    q += [lines.count, lines.count + 1]
    dq = _dev64(q)
    sp = torch.zeros((2, len(q)), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    U.line_spans(hb.ptr, L.N, dq.data_ptr(), len(q), sp[0].data_ptr(), sp[1].data_ptr())
    torch.cuda.synchronize()
    wb, we = lines.spans(q)
    got = sp.cpu().numpy().view(U64)
    assert np.array_equal(got[0], wb) and np.array_equal(got[1], we)
    assert wb[-1] == H.FULL and wb[-2] != H.FULL and any(b <= U64(S) <= e for b, e in zip(wb, we) for S in L.seams)


@pytest.mark.parametrize("invert,files", [(False, False), (True, False), (False, True), (True, True)])
def test_select_lines_bool(U, hb, lined, invert, files):
    """Two oracle lists and the seam list; clauses with a NOT."""
    lines, lists, dlists, _ = lined
    args = [(ds.data_ptr(), dl.data_ptr(), s.size) for (s, _), (ds, dl) in zip(lists, dlists)]
    for clauses in ([(1, 0), (0, 2)], [(1 | 4, 0), (0, 2)], [(2, 0), (4, 1)]):
        want = lines.select_bool(lists, clauses, invert, files)
        sel, nlines, whole = U.select_lines_bool(hb.ptr, L.N, args, clauses, invert, files)
        assert (sel, nlines, whole) == (want[0].size, want[3], want[4]), clauses
        got, out = _line_records(lambda b, e, k, c: U.select_lines_bool(hb.ptr, L.N, args, clauses, invert, files,
                                                                         b, e, k, c), sel)
        assert out == (sel, nlines, whole)
        for g, w in zip(got, want[:3]):
            assert np.array_equal(g, w), clauses


def test_split_matches(U, hb, lined):
    """Bounds ..., S-1, S, S+1, ... N: first, digests, newline and matching-line
    counts per segment, relative offsets and lines per record."""
    lines, _, _, rec = lined
    bounds = [[L.wbase(w) + (5 if w == 0 else 0), S - 1, S, S + 1, L.wend(w)] for w, S in enumerate(L.seams)]
    flat = np.concatenate([np.asarray(b, U64) for b in bounds])
    assert int(flat[-1]) == L.N
    want = lines.split(bounds, rec)
    nseg, m = flat.size - 1, rec[0].size
    db, ds, dl, dc = _dev64(flat), _dev64(rec[0]), _dev32(rec[1]), _dev32(rec[2])
    seg = torch.full((5, nseg + 1), -1, dtype=torch.int64, device="cuda")
    out = torch.full((2, m), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    U.split_matches(hb.ptr, L.N, db.data_ptr(), nseg, ds.data_ptr(), dl.data_ptr(), dc.data_ptr(), 0, m,
                    seg[0].data_ptr(), seg[1].data_ptr(), seg[2].data_ptr(), seg[3].data_ptr(), seg[4].data_ptr(),
                    out[0].data_ptr(), out[1].data_ptr())
    torch.cuda.synchronize()
    s, r = seg.cpu().numpy().view(U64), out.cpu().numpy().view(U64)
    got = {"first": s[0], "digest": s[1, :nseg], "dcap": s[2, :nseg], "newlines": s[3, :nseg], "mlines": s[4, :nseg],
           "rel": r[0], "line": r[1]}
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# --- binary detection ---------------------------------------------------------

def _expect_bad(win, fn):
    """First failing offset of the buffer whose windows hold `win`: the filler
    is clean ASCII, so it is the first window's."""
    r = fn(win)
    return None if r is None else L.wbase(0) + r


def test_utf8_nul_binary_at_the_seams(U, hb, base):
    """A clean buffer is valid; one bad byte or NUL at S-1, S and S+1 of the
    last window, and the split 3- and 4-byte characters cut short, are found
    at their offsets (oracle_lib.utf8_first_bad / first_nul on the window)."""
    def check(win_last, what):
        # the windows differ here: the first one stays clean
        want_u, want_z = utf8_first_bad(win_last), first_nul(win_last)
        want_u = None if want_u is None else L.wbase(LAST) + want_u
        want_z = None if want_z is None else L.wbase(LAST) + want_z
        assert U.check_utf8(hb.ptr, L.N) == want_u, what
        assert U.find_nul(hb.ptr, L.N) == want_z, what
        assert U.is_binary(hb.ptr, L.N) == is_binary(win_last), what
        assert U.is_binary(hb.ptr, L.N, nul_only=True) == is_binary(win_last, nul_only=True), what
        return want_u, want_z

    def put(win):
        hb.buf[L.wbase(LAST):L.wend(LAST)].copy_(torch.from_numpy(np.array(win, dtype=np.uint8)).to("cuda"))
        torch.cuda.synchronize()

    assert utf8_first_bad(base) is None and first_nul(base) is None
    assert check(base, "clean") == (None, None)
    S = L.half
    try:
        for name in ("utf3", "utf4"):
            win = H.variant(L, base, name)
            put(win)
            assert check(win, name) == (None, None)
            lead = S - 1 if name == "utf3" else S - 2
            for cut in range(lead + 1, lead + (3 if name == "utf3" else 4)):   # a continuation byte replaced
                bad = win.copy()
                bad[cut] = ord("x")
                put(bad)
                got = check(bad, (name, cut))
                assert got[0] is not None and abs(got[0] - L.seams[LAST]) <= 3
        for at in (S - 1, S, S + 1):
            for byte in (0xFF, 0x00):
                bad = base.copy()
                bad[at] = byte
                put(bad)
                got = check(bad, (at, byte))
                assert got[0] == L.wbase(LAST) + at and (got[1] == got[0]) == (byte == 0)
        # both windows bad: the first one's offset (past 2^31) is reported
        bad = base.copy()
        bad[S] = 0xFF
        hb.set(bad)
        assert U.check_utf8(hb.ptr, L.N) == _expect_bad(bad, utf8_first_bad) == L.seams[0]
    finally:
        hb.restore()


def test_generator_past_4gib(U):
    """ugpu_gen at off = 2^32 - 1000 equals the oracle's generator."""
    off, n = (1 << 32) - 1000, 4096
    for kind in (1, 2, 3, 4):
        t = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        U.gen(kind, 3, off, t.data_ptr(), n, _stream())
        torch.cuda.synchronize()
        assert np.array_equal(t[:n].cpu().numpy(), gen(kind, 3, off, n)), kind


# --- stream --------------------------------------------------------------------

def test_stream_past_4gib(U, tabs):
    """65 feeds of one host chunk of 64 MiB + 3 bytes: filler with planted
    matches, one split by the chunk edge, one across 2^31 (feed 31) and one
    across 2^32 (feed 63).  The records repeat with the chunk's length, so the
    oracle over two chunks gives them all."""
    t = {x.name: x for x in tabs}["c2_foobarbaz"]
    n, feeds = (64 << 20) + 3, 65
    at31, at32 = (1 << 31) - 31 * n, (1 << 32) - 63 * n   # the seams' offsets in feeds 31 and 63
    assert 0 < at31 < n and 0 < at32 < n
    chunk = H.stream_chunk(n, L.P, [(0, b"z"), (n - 2, b"ba"),          # "baz" split by every chunk edge
                                    (at31 - 1, b"foo"),                  # crosses 2^31
                                    (at32 - 2, b"bar"), (at32 + 1, b"foo"),   # crosses 2^32, starts behind it
                                    (12345, b"foo barbaz"), (n // 2, b"bazfoo")])
    want = H.stream_expected(t, chunk, feeds, 2)
    assert want[0].size == 8 + 9 * (feeds - 1)
    assert np.all(np.diff(want[0].astype(np.int64)) > 0) and int(want[0][-1] + want[1][-1]) <= feeds * n
    assert np.any(want[0] == U64((1 << 31) - 1)) and np.any(want[0] == U64((1 << 32) - 2))
    with t.environ():
        pat = _pattern(U, t)
        s = U.Stream(pat)
        cnt = dg = dc = 0
        listed = []
        for i in range(feeds):
            offsets = i in (31, 32, 63, 64)   # the seam's feed and the next one, which settles its last 64 KiB
            r = s.feed(chunk, final=i == feeds - 1, offsets=offsets)
            if offsets:
                _same(_find_result(r), tuple(x[cnt:cnt + r.count] for x in want), ("feed", i))
                listed += r.start.tolist()
            cnt, dg, dc = cnt + r.count, (dg + r.digest) % (1 << 64), (dc + r.dcap) % (1 << 64)
            assert s.settled() <= (i + 1) * n
        assert s.settled() == feeds * n
        assert {(1 << 31) - 1, (1 << 32) - 2, (1 << 32) + 1, 32 * n - 2, 64 * n - 2} <= set(listed)
        assert (cnt, dg, dc) == H.totals(want, feeds * n)[:3]
        s.close()
    assert oracle_dfa(t.opc).supported
