"""CPU: the layouts of tests/test_open_walks.py (tests/open_walks.py), not the
engine.

The GPU test claims, for every layout, how many open walks fix_kernel's R1
leaves to R1b (Layout.k).  A layout that quietly produced fewer -- a walk that
dies early, a plant that runs into the next one, a range end that is not where
the helper thinks -- would let the GPU test pass without reaching what it is
there for.  So here the record ranges are tied to a restatement of engine.hip
geometry(), the open walks are found from the bytes with the pattern's own
table (the opcode words, parsed by tests/dfa_equiv.py) by a small model of the
COUNT pass's chain, and R1 is restated in Python over them."""
import numpy as np
import pytest

import open_walks as OW
from dfa_equiv import _Table

MAX_REC = 8192            # kMaxRec
MAX_REC_BYTES = 1 << 30   # kMaxRecBytes
SP_WAVES = 4              # kSpWaves
DEAD, CONV, UNRES = 1, 2, 3


def geometry(lo, hi, max_rec, unit=OW.TILE, per=SP_WAVES):
    """engine.hip geometry() for a 16-byte aligned buffer (off = 0): the byte
    ranges of the chain records."""
    t0 = lo // unit
    t1 = (hi + unit - 1) // unit
    if t1 <= t0:
        t1 = t0 + 1
    nt = t1 - t0
    nrec = max(min(nt, max_rec), 1)
    min_rec = (nt * unit + MAX_REC_BYTES - 1) // MAX_REC_BYTES
    if nrec < min_rec:
        nrec = min(min_rec, nt)
    tpr = (nt + nrec - 1) // nrec
    nrec = (nt + tpr - 1) // tpr
    grid = (nrec + per - 1) // per
    out = []
    for b in range(grid * per):
        tb = t0 + b * tpr
        te = min(tb + tpr, t1)
        tb = min(tb, te)
        out.append((min(max(tb * unit, lo), hi), min(max(te * unit, lo), hi)))
    return out


@pytest.fixture(scope="module")
def U():
    import ugrep_amd
    return ugrep_amd


_TABLES = {}


def _table(U, rx):
    if rx not in _TABLES:
        t = _Table(U.compile_regex(rx))
        nxt = [[t.norm(s) for s in row] for row in t.next.tolist()]
        _TABLES[rx] = (nxt, t.caps.tolist(), t.start)
    return _TABLES[rx]


def _walk(nxt, caps, s, data, pos):
    """The walk in state s over data (bytes starting at position pos): (state
    at the end or 0, position it stopped before, end of the last accept or 0)."""
    last = 0
    for c in data:
        s = nxt[s][c]
        if not s:
            return 0, pos, last
        pos += 1
        if caps[s]:
            last = pos
    return s, pos, last


def _count_pass(U, lay):
    """The COUNT pass's speculative chains, for these layouts: per record the
    first kept match start (or None), and its open walk (c, lim, state at lim)
    when the chain ends in a walk alive kOpenSlack past the range end."""
    nxt, caps, start = _table(U, lay.rx)
    rend = lay.n + lay.tail
    raw = lay.host.tobytes()
    firsts = np.flatnonzero(np.array([nxt[start][c] != 0 for c in range(256)])[lay.host[:lay.n]])
    first, opened = {}, {}
    for b in range(lay.nrec):
        lo, hi = lay.range_start(b), lay.range_end(b)
        lim = rend if hi >= lay.n else min(hi + OW.SLACK, rend)
        p = lo
        for c in firsts[np.searchsorted(firsts, lo):np.searchsorted(firsts, hi)].tolist():
            if c < p:
                continue
            s, _, last = _walk(nxt, caps, start, raw[c:lim], c)
            if s and lim < rend:
                first.setdefault(b, c)
                opened[b] = (c, lim, s)
                break
            if last:
                first.setdefault(b, c)
                p = last
            else:
                p = c + 1
    return first, opened


def _r1(U, lay, first, opened):
    """fix_kernel's R1 (scan_kernels.hip resolve_open) restated: the type of each open walk."""
    nxt, caps, start = _table(U, lay.rx)
    rend = lay.n + lay.tail
    h = lay.host.tobytes()
    types = {}
    for b, (c, q, s) in opened.items():
        c1 = first.get(b + 1)
        qmax = q + OW.CONV
        v = 0
        if c1 is not None and c1 < q:
            v = _walk(nxt, caps, start, h[c1:q], c1)[0]
        while True:
            if q == c1:
                v = start
            if v and v == s:
                types[b] = CONV
                break
            if q >= rend:
                types[b] = DEAD
                break
            if q >= qmax:
                types[b] = UNRES
                break
            s = nxt[s][h[q]]
            if v:
                v = nxt[v][h[q]]
            if not s:
                types[b] = DEAD
                break
            q += 1
    return types


_MODEL = {}


def _model(U, name):
    if name not in _MODEL:
        lay = OW.layout(name)
        first, opened = _count_pass(U, lay)
        _MODEL[name] = (first, opened, _r1(U, lay, first, opened))
    return _MODEL[name]


@pytest.mark.parametrize("rx", [OW.RX, OW.RX2, OW.RX5])
def test_letters_keep_a_walk_alive(U, rx):
    """The pattern's own loop: after `x`, every letter keeps the walk alive, in
    every state letters lead to; the filler and the blank end it at once."""
    nxt, caps, start = _table(U, rx)
    assert U.host_plan(U.compile_regex(rx))["kernel"] == 0
    assert [c for c in range(256) if nxt[start][c]] == [ord("x")]
    seen, todo = set(), [nxt[start][ord("x")]]
    while todo:
        s = todo.pop()
        if s in seen:
            continue
        seen.add(s)
        for c in range(ord("a"), ord("z") + 1):
            assert nxt[s][c], (rx, s, chr(c))
            todo.append(nxt[s][c])
        assert not any(nxt[s][c] for c in OW.FILL)
        z = nxt[s][ord("Z")]
        assert bool(z) == (rx == OW.RX2) and (not z or (caps[z] and not any(nxt[z])))
    assert len(seen) >= (5 if rx == OW.RX5 else 1)


@pytest.mark.parametrize("name", list(OW.CASES))
def test_ranges_are_the_engines(name):
    lay = OW.layout(name)
    want = geometry(0, lay.n, lay.grid)
    assert [r for r in want if r[0] < r[1]] == [(lay.range_start(b), lay.range_end(b)) for b in range(lay.nrec)]
    assert lay.rec % OW.TILE == 0 and lay.n <= (80 << 20)
    assert lay.n <= (16 << 20) or name.startswith("budget")
    if name in ("split256", "split257"):
        assert (lay.n, lay.grid, lay.rec) == (16 << 20, 512, 32 << 10)


@pytest.mark.parametrize("name", list(OW.CASES))
def test_plants_stand_alone(name):
    """Each plant's letters end before the next plant, nothing else in the
    buffer starts a walk, and each is long enough for R1 to give it up."""
    lay = OW.layout(name)
    h = lay.host
    letter = (h >= ord("a")) & (h <= ord("z"))
    inside = np.zeros(h.size, bool)
    prev = -1
    for p in lay.plants:
        assert p.end == lay.range_end(p.rec) and (p.end - p.x) in OW.D
        assert prev < p.x and h[p.x] == ord("x")
        assert letter[p.x + 1:p.die].all() and (p.die == h.size or not letter[p.die])
        assert p.die > p.r1_end, "R1 could finish this walk"
        assert p.rec < lay.nrec - 1
        inside[p.x:p.die] = True
        prev = p.die
    assert not (letter & ~inside).any()
    if name != "chains":
        assert int((h == ord("x")).sum()) == len(lay.plants)


@pytest.mark.parametrize("name", list(OW.CASES))
def test_unresolved_walks(U, name):
    """The walks R1 leaves to R1b are as many as the GPU test claims, and they
    are the plants'."""
    lay = OW.layout(name)
    first, opened, types = _model(U, name)
    unres = sorted(b for b, t in types.items() if t == UNRES)
    assert len(unres) == lay.k
    longest = max(p.die - p.r1_end for p in lay.plants)
    assert lay.forest == (lay.k > OW.COOP_MAX or longest > OW.COOP_BUDGET)
    if name == "chains":
        assert unres == [last for _, last, _ in lay.runs]
        assert sorted(opened) == [r for b, last, _ in lay.runs for r in range(b, last + 1)]
        assert all(types[r] == CONV for r in opened if r not in unres)
    else:
        assert unres == [p.rec for p in lay.plants] == sorted(opened)
        assert [opened[p.rec][0] for p in lay.plants] == [p.x for p in lay.plants]


@pytest.mark.parametrize("name", list(OW.CASES))
def test_matches_fit_the_stitch_rounds(U, name):
    """fix_kernel hands a match's end to the records it covers one round at a
    time and gives up after fix_rounds_for() rounds (engine.hip: 256 KiB / the
    record size, 4 to 16): no match of a layout that expects to stay off the
    forest FIND covers that many records, so its FOREST flag speaks of R1b."""
    from oracle_lib import OracleDfa
    lay = OW.layout(name)
    if lay.forest:
        return
    rounds = min(max((256 << 10) // lay.rec, 4), 16)
    st, ln, _ = OracleDfa(U.compile_regex(lay.rx)).find_arrays(lay.host)
    crossed = ((st + ln - np.uint64(1)) // np.uint64(lay.rec) - st // np.uint64(lay.rec)).tolist()
    if name == "chains":    # (the records of a run have open walks of their own: the ones behind its last)
        crossed = [(p.die - 1) // lay.rec - last for _, last, p in lay.runs]
    assert max(crossed, default=0) < rounds


def test_wave_split_lengths():
    """4.5 KiB to 200 KiB, not in order of length, more walks than waves from K = 17 on."""
    for K in OW.SPLIT_K:
        lay = OW.layout("split%d" % K)
        L = [p.die - p.x - 1 for p in lay.plants]
        assert len(L) == K and min(L) >= 4608 and max(L) <= 200 << 10
        if K >= 16:
            assert min(L) == 4608 and max(L) == 200 << 10 and L != sorted(L) and L != sorted(L, reverse=True)
    assert [K for K in OW.SPLIT_K if K > OW.COOP_MAX] == [OW.COOP_MAX + 1] and OW.COOP_MAX in OW.SPLIT_K
    for name, over in (("budget63", False), ("budget", True)):
        p = OW.layout(name).plants[0]
        assert (p.die - p.r1_end > OW.COOP_BUDGET) == over and abs(p.die - p.r1_end - OW.COOP_BUDGET) <= (1 << 20) + 8192
        assert not (OW.layout(name).host[p.x:p.die] == ord("y")).any()


def test_where_the_last_accept_lies(U):
    """The seven places of the `accepts` layout, from the bytes: the end of each plant's match."""
    lay = OW.layout("accepts")
    nxt, caps, start = _table(U, lay.rx)
    raw = lay.host.tobytes()
    seen = set()
    for i, p in enumerate(lay.plants):
        s, pos, last = _walk(nxt, caps, start, raw[p.x:p.die + 1], p.x)
        assert not s and pos == p.die
        cat = i % OW.ACCEPT_CASES
        q0 = p.r1_end
        fr = q0 + (p.die - q0) // 1024 * 1024
        assert [last == 0, p.x < last <= p.end, p.end < last <= p.end + OW.SLACK, p.end + OW.SLACK < last <= q0,
                q0 < last < p.die, max(fr, q0) < last < p.die and p.die - fr < 1024, last == p.die][cat], (i, cat)
        seen.add(cat)
    assert seen == set(range(OW.ACCEPT_CASES))
    # both edges of the slack and of R1's budget
    ends = {_walk(nxt, caps, start, raw[p.x:p.die + 1], p.x)[2] - p.end for p in lay.plants}
    assert {1, OW.SLACK, OW.SLACK + 1, OW.SLACK + OW.CONV} <= ends


def test_accept_indices_and_phases(U):
    """acceptsZ ends walks on both accept indices; guess5 has `y` at phases that accept and that do not."""
    from oracle_lib import OracleDfa
    lay = OW.layout("acceptsZ")
    lst = OracleDfa(U.compile_regex(lay.rx)).find(lay.host, want_list=True)[3]
    by_start = {s: (ln, cap) for s, ln, cap in lst}
    caps = [by_start[p.x][1] for p in lay.plants if p.x in by_start]
    assert set(caps) == {1, 2} and len(caps) >= len(lay.plants) - 3
    assert all(by_start[p.x] == (p.die + 1 - p.x, 2) for i, p in enumerate(lay.plants) if i % 2)
    lay = OW.layout("guess5")
    cnt = OracleDfa(U.compile_regex(lay.rx)).find(lay.host)[0]
    assert cnt == sum(1 for i in range(len(lay.plants)) if i % 3) and 0 < cnt < len(lay.plants)
    assert int((lay.host == ord("y")).sum()) >= 3 * len(lay.plants)


def test_chains_cross_a_group_of_64():
    """R2 takes the open records 64 at a time: runs lie across its group
    borders, and a run without `y` is among them."""
    lay = OW.layout("chains")
    assert len(lay.runs) == 20
    assert sum(1 for b, last, _ in lay.runs if b // 64 != last // 64) >= 3
    noy = [(b, last) for b, last, p in lay.runs if not (lay.host[p.x:p.die] == ord("y")).any()]
    assert len(noy) == 5 and any(b // 64 != last // 64 for b, last in noy)
    for b, last, p in lay.runs:
        ys = np.flatnonzero(lay.host[p.x:p.die] == ord("y")) + p.x
        assert ys.size <= 1 and (ys > lay.range_end(last) + OW.SLACK + OW.CONV).all()
