"""CPU: the references of tests/test_highpos.py (tests/highpos.py) on a layout
small enough to check them against the plain ones.

The GPU test cannot run the oracle or the numpy line models over its 4 GiB
buffer; it folds them from one 2 MiB window.  Here the same layout is built
with seams at 2^19 and 2^20, a period of 4 KiB and windows of 128 KiB, the
whole buffer is materialised, and every folded reference must equal the oracle
and the models run over all of it.  The planted bytes must give every table a
record on each side of the seam, and the table list must reach every kernel."""
import json
import os

import numpy as np
import pytest

import batch_model
import boolsel_model
import highpos as H
import linesel_model
from oracle_lib import GOLDEN, first_nul, gen, utf8_first_bad
from ugrep_amd._lib import SHAPE_FILTER2, SHAPE_LOOKAHEAD, SHAPE_LOOP_NEEDLE

L = H.small_layout()


@pytest.fixture(scope="module")
def U():
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def tabs(U):
    with open(os.path.join(GOLDEN, "patterns.json")) as f:
        return H.tables(U, json.load(f))


@pytest.fixture(scope="module")
def base():
    b = H.base_window(L)
    b.setflags(write=False)
    return b


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_layout(base):
    whole = L.whole(base)
    assert whole.size == L.N == (1 << 20) + (64 << 10)
    for w, S in enumerate(L.seams):
        assert whole[L.wbase(w) - 1] == 10 and whole[L.wend(w) - 1] == 10
        assert L.newlines_before(w, base) == int(np.count_nonzero(whole[:L.wbase(w)] == 10))
    F = H.full_layout()
    assert F.N == (1 << 32) + (1 << 20) and F.wbase(0) % F.P == 0 and F.wbase(1) == (1 << 32) - (1 << 20)
    assert F.newlines_before(1, np.zeros(0, np.uint8)) == 4095 - 2   # (the issue's 4095, less window A's two periods)
    assert chr(H.F).isprintable() and not chr(H.F).isalnum() and chr(H.F) not in "_ \n"


def test_plan_reaches_every_kernel_and_shape(U, tabs):
    seen, shapes = set(), {}
    assert len(tabs) == H.N_TABLES and tuple(i for i, t in enumerate(tabs) if t.both) == H.BOTH
    assert all(t.both == (t.kernel in (0, 1, 5, 6)) for t in tabs) and all(len(t.variants) >= 4 for t in tabs)
    for t in tabs:
        info = t.plan(U)
        assert info["kernel"] == t.kernel, t.name
        seen.add(info["kernel"])
        shapes[t.name] = info
    assert seen == set(range(8))
    assert shapes["c2_foobarbaz"]["shape"] & SHAPE_FILTER2
    assert not shapes["c2_foobarbaz/ft2=0"]["shape"] & SHAPE_FILTER2
    assert shapes["[a-z]+ing"]["shape"] & SHAPE_LOOP_NEEDLE
    assert shapes["foo(?= bar)"]["shape"] & SHAPE_LOOKAHEAD
    assert shapes[r"\bfoo\b"]["contexts"] == 64 and shapes[r"\<(in|ut)\>"]["contexts"] == 64   # context walks
    assert shapes["^foo"]["contexts"] == 4
    # option W on the sparse kernel, on wfind_kernel, on xc_kernel and on the n-gram kernel
    assert {t.kernel for t in tabs if t.word} == {0, 4, 5, 7}
    # what host_plan reports about option W (the info has no W bit of its own): the plan changes with it.
    # W drops FILTER2 and keeps foo|bar|baz on the sparse kernel only through WSPARSE; the word pair
    # table leaves the dense kernel for wfind_kernel; [A-Za-z]+ keeps xc_kernel (its W mode)
    by = {t.name: t for t in tabs}
    w = by["foo|bar|baz -w"]
    assert not shapes[w.name]["shape"] & SHAPE_FILTER2 and U.host_plan(w.opc)["shape"] & SHAPE_FILTER2
    with w.environ(UGPU_WSPARSE=0, UGPU_SPARSE=0):
        assert U.host_plan(w.opc, word=True)["kernel"] == 4
    assert U.host_plan(by["[a-z_0-9é日本]{2} -w"].opc)["kernel"] != 4
    assert {t.name for t in tabs if not H.dead_on_filler(L, t)} == {r"\D\D"}


def test_planted_bytes_meet_every_table(tabs, base):
    """end / start / cross: a record that ends at the seam, starts at it, and
    starts one byte before it, in the chain of the whole buffer."""
    S = L.half
    for t in tabs:
        got = {}
        for name in ("end", "start", "cross"):
            st, ln, _ = H.records(t, H.variant(L, base, name, t), 0)
            got[name] = (st.astype(np.int64), ln.astype(np.int64))
        assert np.any(got["end"][0] + got["end"][1] == S), t.name
        assert np.any(got["start"][0] == S), t.name
        k = np.flatnonzero(got["cross"][0] == S - 1)
        assert k.size and got["cross"][1][k[0]] >= 2, t.name


def test_run_and_split_characters(tabs, base):
    by = {t.name: t for t in tabs}
    S = L.half
    run = H.variant(L, base, "run")
    assert np.all(run[S - L.run // 2:S + L.run // 2 - 1] == ord("a")) and L.run >= 20 << 10
    assert H.full_layout().run >= 300 << 10
    st, ln, _ = H.records(by["a+"], run, 0)
    assert L.run in ln.tolist()
    st, ln, _ = H.records(by["[a-z]+ing"], H.variant(L, base, "lbrun"), 0)
    assert np.any((st == np.uint64(S - 4096)) & (ln == np.uint64(8195)))
    for name, lead, nb in (("utf3", 0xE6, 3), ("utf4", 0xF0, 4)):
        v = H.variant(L, base, name)
        k = S - 1 if nb == 3 else S - 2
        assert v[k] == lead and all(0x80 <= x < 0xC0 for x in v[k + 1:k + nb])
        st, ln, _ = H.records(by["c4_word"], v, 0)   # the split character lies inside one \w+ match
        assert np.any((st.astype(np.int64) < k) & (st.astype(np.int64) + ln.astype(np.int64) > k + nb)), name
    v = H.variant(L, base, "nl")
    assert v[S - 1] == 10 and v[S] == 10
    v = H.variant(L, base, "crlf")
    assert v[S - 1] == 13 and v[S] == 10


@pytest.mark.parametrize("name", ["end", "start", "cross", "run", "lbrun", "utf3", "utf4"])
def test_folded_find_equals_whole_buffer_oracle(tabs, base, name):
    for t in tabs:
        if name not in t.variants:
            continue
        win = H.variant(L, base, name, t)
        whole = L.whole(win)
        dead = H.dead_on_filler(L, t)
        if dead:
            assert _same(H.folded_records(L, t, win, 0, None), H.records(t, whole, 0)), t.name
        for w in range(len(L.seams)):
            cur = L.wbase(w) + 1                     # find_all from a cursor
            if dead:
                assert _same(H.folded_records(L, t, win, w, cur), H.records(t, whole, cur)), (t.name, w)
            for lo, hi in H.scan_ranges(L, w):
                f = H.folded_records(L, t, win, w, lo)
                p = H.records(t, whole, lo)
                assert H.totals(f, hi) == H.totals(p, hi), (t.name, w, lo, hi)
                assert H.totals(f, hi, 1 << 40) == H.totals(p, hi, 1 << 40), (t.name, w, lo, hi)
                assert _same(H.head(f, hi), H.head(p, hi)), (t.name, w, lo, hi)


def _lists(tabs, win):
    """Match lists of the whole buffer for the line consumers: two oracle
    lists and the hand-made seam list."""
    by = {t.name: t for t in tabs}
    a = H.folded_records(L, by["c3_ident"], win, 0, None)
    b = H.folded_records(L, by["c2_foobarbaz"], win, 0, None)
    return [(a[0], a[1]), (b[0], b[1]), H.seam_list(L)]


@pytest.mark.parametrize("name", ["nl", "crlf"])
def test_folded_line_models_equal_whole_buffer_models(tabs, base, name):
    win = H.variant(L, base, name)
    whole = L.whole(win)
    lines = H.Lines(L, win)
    lists = _lists(tabs, win)
    wb, we = linesel_model.line_table(whole)
    assert np.array_equal(lines.begin, wb.astype(np.uint64)) and np.array_equal(lines.end, we.astype(np.uint64))
    for s, ln in lists + [(lists[2][0], None)]:
        for inv in (False, True):
            got = lines.select(s, ln, inv)
            want = linesel_model.select(whole, s.astype(np.int64), None if ln is None else ln.astype(np.int64), inv)
            assert _same(got[:3], want[:3]) and got[3] == want[3]
        nl, ml, line = lines.line_of(s)
        nlpos = np.flatnonzero(whole == 10)
        wline = np.searchsorted(nlpos, s.astype(np.int64), side="left") + 1
        assert nl == nlpos.size and np.array_equal(line, wline.astype(np.uint64)) and ml == np.unique(wline).size
    ilists = [(s.astype(np.int64), ln.astype(np.int64)) for s, ln in lists]
    for clauses in ([(1, 0), (0, 2)], [(1 | 4, 0), (0, 2)], [(0, 1)], [(2, 0), (4, 1)]):
        for inv in (False, True):
            for files in (False, True):
                got = lines.select_bool(lists, clauses, inv, files)
                want = boolsel_model.select(whole, ilists, clauses, inv, files)
                assert _same(got[:3], want[:3]) and got[3:] == want[3:], (clauses, inv, files)
    q = []
    for w, S in enumerate(L.seams):
        k = int(lines.line_of(np.asarray([S], np.uint64))[2][0])
        q += [k - 1, k, k + 1, k + 2]
    q += [lines.count, lines.count + 1]
    assert _same(lines.spans(q), linesel_model.spans(whole, q))
    rec = H.folded_records(L, {t.name: t for t in tabs}["c3_ident"], win, 0, None)
    bounds = [[L.wbase(w) + (5 if w == 0 else 0), S - 1, S, S + 1, L.wend(w)] for w, S in enumerate(L.seams)]
    got = lines.split(bounds, rec)
    want = batch_model.split(whole, np.concatenate([np.asarray(b, np.uint64) for b in bounds]), *rec)
    for k in want:
        assert np.array_equal(got[k], want[k].astype(np.uint64)), k


def test_generator_offsets_past_4gib():
    """The oracle's corpus generator at offsets around 2^32: a range equals the
    same bytes taken from ranges that start elsewhere."""
    off, n = (1 << 32) - 1000, 4096
    for kind in (1, 2, 3, 4):
        a = gen(kind, 3, off, n)
        assert np.array_equal(a, gen(kind, 3, off - 77, n + 77)[77:]), kind
        assert np.array_equal(a[1000:], gen(kind, 3, 1 << 32, n - 1000)), kind
        assert not np.array_equal(a, gen(kind, 3, off - (1 << 32), n)), kind   # (no wrap at 32 bits)


def test_folded_binary_checks(base):
    """The first bad byte or NUL of the buffer is the first bad window's."""
    assert utf8_first_bad(L.whole(base)) is None and first_nul(L.whole(base)) is None
    for name in ("utf3", "utf4", "nl", "crlf"):
        assert utf8_first_bad(L.whole(H.variant(L, base, name))) is None, name
    for at, byte in ((L.half - 1, 0xFF), (L.half, 0), (L.half + 1, 0x80)):
        bad = base.copy()
        bad[at] = byte
        whole = L.whole(base)
        whole[L.wbase(1):L.wend(1)] = bad             # the last window alone
        assert utf8_first_bad(whole) == L.wbase(1) + utf8_first_bad(bad) == L.wbase(1) + at
        assert first_nul(whole) == (L.wbase(1) + at if byte == 0 else None)
        assert utf8_first_bad(L.whole(bad)) == L.wbase(0) + at   # both windows: the first one's


def test_stream_reference_repeats_with_the_chunk(tabs):
    """highpos.stream_expected (two chunks, tiled) equals the oracle over all the chunks."""
    t = {x.name: x for x in tabs}["c2_foobarbaz"]
    n, feeds = 4096 + 3, 7
    chunk = H.stream_chunk(n, 512, [(0, b"z"), (n - 2, b"ba"), (n - 97, b"foo"), (n - 194, b"bar"), (n - 191, b"foo"),
                                    (1234, b"foo barbaz"), (n // 2, b"bazfoo")])
    want = H.stream_expected(t, chunk, feeds, 2)
    assert _same(want, H.records(t, np.concatenate([chunk] * feeds), 0))
    assert want[0].size == 8 + 9 * (feeds - 1)
