"""Layout, tables and references of the high-offset tests (tests/test_highpos.py
on the GPU, tests/test_highpos_host.py on the CPU).

One buffer of N bytes is filler -- byte F, with '\\n' closing every period of P
bytes -- except for two windows [S - half, S + half) around two seams S (2^31
and 2^32 at full scale).  Both windows hold the same bytes: a mixed corpus with
a patch ("variant") at the seam.  Nothing outside the windows can match a table
that is dead on filler, and every line outside them is a filler line, so the
records of the whole buffer follow from the oracle and the numpy line models
run on one window alone ("folded" references): offsets move by the window's
base, line numbers by the lines before it.  The CPU test builds the same layout
small enough to run the oracle and the models over the whole buffer, and
asserts that the folded references equal those.

No code under test computes an expected value here: host_plan() is only read
for the kernel a table runs on.
"""
import contextlib
import os

import numpy as np

import batch_model
import boolsel_model
import linesel_model
import wordset_gen
from oracle_lib import gen, oracle_dfa

F = ord(".")
U64 = np.uint64
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)


class Layout:
    def __init__(self, seams, period, half, run, rhalf):
        self.seams, self.P, self.half, self.run, self.rhalf = list(seams), period, half, run, rhalf
        self.N = self.seams[-1] + half
        assert all((s - half) % period == 0 and (s + half) % period == 0 for s in self.seams)
        assert self.seams == sorted(self.seams) and run + 64 < 2 * rhalf < 2 * half

    def wbase(self, w):
        return self.seams[w] - self.half

    def wend(self, w):
        return self.seams[w] + self.half

    def newlines_before(self, w, win):
        """'\\n' bytes in [0, wbase(w)) when every window holds `win`."""
        k = int(np.count_nonzero(win == 10))
        return (self.wbase(w) - 2 * self.half * w) // self.P + k * w

    def whole(self, win):
        """The whole buffer on the host (small layouts only)."""
        buf = np.full(self.N, F, np.uint8)
        buf[self.P - 1::self.P] = 10
        for w in range(len(self.seams)):
            buf[self.wbase(w):self.wend(w)] = win
        return buf

    def filler(self, n=4096):
        """n bytes of filler around one of its newlines."""
        buf = np.full(n, F, np.uint8)
        buf[n // 2] = 10
        return buf


def full_layout():
    """Seams at 2^31 and 2^32, windows of 2 MiB, N = 2^32 + 1 MiB."""
    return Layout([1 << 31, 1 << 32], 1 << 20, 1 << 20, 304 << 10, 300001)


def small_layout():
    """The same shape at seams 2^19 and 2^20 for the CPU test."""
    return Layout([1 << 19, 1 << 20], 4096, 64 << 10, 20 << 10, 20001)


def base_window(L):
    """The windows' corpus: slices of the UTF-8 word, code and word corpora,
    closed by a stretch of filler and a '\\n' (so a window ends like a filler
    period and no match of a filler-dead table lies at its end)."""
    n = 2 * L.half
    win = np.concatenate([gen(4, 7, 0, 3 * n // 8), gen(3, 7, 0, 3 * n // 8), gen(1, 7, 0, n // 4)])
    assert win.size == n
    win[-256:] = F
    win[-1] = 10
    return win


# --- the planted bytes -------------------------------------------------------
# SAMPLE is free of context: its head "\n0\n" ends every open match and resets
# the phase of tables whose chains do not resynchronise on text (a digit is
# dead for \D\D), so its matches from offset 3 on are the same wherever it
# lies.  Its tail "\n0\n" does the same for the bytes behind it.
_WORDS = wordset_gen.words(300)
SAMPLE = ("\n0\nfoo bar baz in ut sing ring aaaa 12 345 ab cd_ef x1 foo bar café 日本 Hello World "
          + " ".join(_WORDS[i] for i in (0, 3, 7, 150, 299)) + " foo bar\nfoo baz\nfoo\n0\n").encode()


def _patch(win, at, data):
    data = np.frombuffer(bytes(data), np.uint8)
    assert 0 <= at and at + data.size <= win.size - 256
    win[at:at + data.size] = data


def variant(L, base, name, tab=None):
    """A copy of the base window with the seam patch `name`; the seam is at
    window offset L.half.
      end / start / cross   SAMPLE placed so that one match of `tab` ends at
                            the seam, starts at it, or starts one byte before it
      run                   L.run bytes of 'a' centred on the seam
      lbrun                 8 KiB of 'a' centred on the seam, then "ing"
      utf3 / utf4           a 3-byte / 4-byte word character split by the seam
      nl / crlf             '\\n' at S-1 and S / "\\r\\n" split by the seam"""
    win = base.copy()
    S = L.half
    if name in ("end", "start", "cross"):
        s, ln = sample_match(tab)
        _patch(win, {"end": S - (s + ln), "start": S - s, "cross": S - s - 1}[name], SAMPLE)
    elif name == "run":
        _patch(win, S - L.run // 2 - 1, b" " + b"a" * L.run + b" ")
    elif name == "lbrun":
        _patch(win, S - 4097, b" " + b"a" * 8192 + b"ing ")
    elif name == "utf3":
        _patch(win, S - 7, " abéx日本y cd ".encode())      # E6 | 97 A5
    elif name == "utf4":
        _patch(win, S - 6, " abx\U0001D400éy cd ".encode())        # F0 9D | 90 80
    elif name == "nl":
        _patch(win, S - 9, b"foo x_1 \n\nbar y2\n")
    elif name == "crlf":
        _patch(win, S - 8, b"foo x_1\r\nbar y2\r\n")
    else:
        raise ValueError(name)
    return win


def sample_match(tab):
    """(start, len) in SAMPLE of the match of `tab` that the end / start / cross
    variants put on the seam: the first one past the head with two bytes or more."""
    st, ln, _ = records(tab, np.frombuffer(SAMPLE, np.uint8), 0)
    ok = np.flatnonzero((st >= 3) & (ln >= 2))
    assert ok.size, tab.name
    return int(st[ok[0]]), int(ln[ok[0]])


# --- the tables --------------------------------------------------------------

class Table:
    def __init__(self, name, kernel, opc, word=False, env=None, both=False, variants=(), stage=False, run="run",
                 slow_run=False):
        self.name, self.kernel, self.word, self.env = name, kernel, word, dict(env or {})
        self.opc = np.ascontiguousarray(np.asarray(opc, np.uint32))
        self.both = both                                  # both windows (kernels 0, 1, 5, 6)
        self.variants = ("end", "start", "cross", run) + tuple(variants)
        self.stage = stage                                # sparse tables: staged and rebuilt records
        self.slow_run = slow_run                          # the 304 KiB run is one match: 0.3 to 1.5 s per scan

    def __repr__(self):
        return self.name

    @contextlib.contextmanager
    def environ(self, **more):
        """The table's knobs (and `more`) in the environment."""
        env = dict(self.env, **{k: str(v) for k, v in more.items()})
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            yield
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    def plan(self, U):
        with self.environ():
            return U.host_plan(self.opc, word=self.word)


FOREST = {"UGPU_FIX_BUDGET": "1", "UGPU_MERGE_BUDGET": "1"}
_U = ("utf3", "utf4")

# The matrix: every kernel id 0 to 7 and the shapes the issue names.
# (name, kernel, source, options): source is a regex, ("pat", key) for a table
# of tests/golden/patterns.json, or "wordset" for the 300-word set.  both: both
# windows (every table of kernels 0, 1, 5 and 6).
SPECS = [
    ("c2_foobarbaz", 0, ("pat", "c2_foobarbaz"), dict(both=True, stage=True)),                       # FILTER2
    ("c2_foobarbaz/ft2=0", 0, ("pat", "c2_foobarbaz"), dict(env={"UGPU_FT2": "0"}, both=True, stage=True)),
    (r"\bfoo\b", 0, r"\bfoo\b", dict(both=True, stage=True)),                                       # context walks
    (r"\<(in|ut)\>", 0, r"\<(in|ut)\>", dict(both=True, stage=True)),
    ("foo|bar|baz -w", 0, "foo|bar|baz", dict(word=True, both=True, stage=True)),                    # W, WSPARSE
    # loop needle.  Its long walk is lbrun: over the run variant the oracle's FIND walks from each of
    # the 300 K positions of the run to its end (4.6e10 steps at full scale; 1.3 s for a run of 20 KiB)
    ("[a-z]+ing", 0, "[a-z]+ing", dict(both=True, stage=True, run="lbrun")),
    ("a+", 0, "a+", dict(both=True, stage=True)),                                                    # long walks
    (r"\D\D", 1, r"\D\D", dict(both=True)),                                                         # forest by itself
    ("aa/dense", 1, ("pat", "aa"), dict(env={"UGPU_SPARSE": "0"}, both=True)),
    # every stitch on the forest FIND.  lbrun: over the 304 KiB run each of its scans takes 1 to 2.8 s
    # on an MI355X (the forest walks one match serially); \D\D and aa/dense reach the forest on that run
    ("c4_word/forest", 1, ("pat", "c4_word"),
     dict(env=dict(FOREST, UGPU_XU="0", UGPU_XG="0"), both=True, variants=_U, run="lbrun")),
    ("c3_ident/xi", 2, ("pat", "c3_ident"), dict(env={"UGPU_XC": "0"}, slow_run=True)),
    ("c4_word/xg", 3, ("pat", "c4_word"), dict(env={"UGPU_XU": "0"}, variants=_U, slow_run=True)),
    ("[a-z_0-9é日本]{2} -w", 4, "[a-z_0-9é日本]{2}", dict(word=True, variants=_U)),
    ("c3_ident", 5, ("pat", "c3_ident"), dict(both=True, variants=_U, slow_run=True)),
    # U mode: the fast kernel, the exact kernel after a UMIX flag, the table's next kernel after USLOW
    ("c4_word", 6, ("pat", "c4_word"), dict(env={"UGPU_XU": "1"}, both=True, variants=_U, slow_run=True)),
    ("[A-Za-z]+ -w", 5, "[A-Za-z]+", dict(word=True, both=True, variants=_U, slow_run=True)),
    ("wordset300", 7, "wordset", {}),
    ("wordset300 -w", 7, "wordset", dict(word=True)),
    ("^foo", 0, "^foo", dict(both=True, stage=True)),
    ("foo(?= bar)", 4, "foo(?= bar)", {}),
]
N_TABLES = len(SPECS)
BOTH = tuple(i for i, sp in enumerate(SPECS) if sp[3].get("both"))


def tables(U, patterns):
    """The Table of every entry of SPECS."""
    out = []
    for name, kernel, src, opt in SPECS:
        if isinstance(src, tuple):
            opc = patterns[src[1]]["opc"]
        else:
            opc = U.compile_regex(wordset_gen.regex(_WORDS) if src == "wordset" else src)
        out.append(Table(name, kernel, opc, **opt))
    return out


# --- FIND references ---------------------------------------------------------

def records(tab, data, start):
    """The oracle's records (start, len, cap as uint64 arrays) of the FIND chain
    entering `data` at `start`."""
    o = oracle_dfa(tab.opc)
    assert o.supported, tab.name
    if tab.word:
        lst = o.find_w(data, start=start, want_list=True)[3]
    elif o.anchored:
        lst = o.find(data, start=start, want_list=True)[3]
    else:
        return o.find_arrays(data, start=start)
    a = np.asarray(lst, dtype=U64).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def shift(rec, by):
    return rec[0] + U64(by), rec[1], rec[2]


def concat(recs):
    return tuple(np.concatenate([r[i] for r in recs]) for i in range(3))


def totals(rec, hi, bias=0):
    """(count, digest, dcap, exit) of a scan to `hi` whose chain has the records
    `rec` (in buffer offsets): the matches that start before hi, exit = the end
    of the last one when it runs past hi, else hi; the digests take start + bias."""
    st, ln, cp = rec
    k = int(np.searchsorted(st, U64(hi), side="left"))
    if not k:
        return 0, 0, 0, hi
    s, l, c = st[:k] + U64(bias), ln[:k], cp[:k]
    with np.errstate(over="ignore"):
        dg = int((s * U64(31) + l).sum(dtype=U64))
        dc = int(((s + U64(1)) * c).sum(dtype=U64))
    end = int(st[k - 1]) + int(ln[k - 1])
    return k, dg, dc, max(end, hi)


def head(rec, hi):
    k = int(np.searchsorted(rec[0], U64(hi), side="left"))
    return rec[0][:k], rec[1][:k], rec[2][:k]


def dead_on_filler(L, tab):
    """No match in a stretch of filler: the table's whole-buffer records are
    those of its windows."""
    return records(tab, L.filler(), 0)[0].size == 0


def folded_records(L, tab, win, w, lo):
    """Records, in buffer offsets, of the chain that enters the buffer at `lo`
    inside window w (or at 0 with lo None) and runs to the end of the buffer.
    Tables that match filler get the chain of window w alone."""
    if lo is None:
        assert dead_on_filler(L, tab)
        one = records(tab, win, 0)
        return concat([shift(one, L.wbase(v)) for v in range(len(L.seams))])
    assert L.wbase(w) <= lo < L.wend(w)
    out = [shift(records(tab, win, lo - L.wbase(w)), L.wbase(w))]
    if dead_on_filler(L, tab):
        one = records(tab, win, 0)
        out += [shift(one, L.wbase(v)) for v in range(w + 1, len(L.seams))]
    return concat(out)


def scan_plan(group, tab):
    """(range index, UGPU_MAX_GRID or None, bias) of the Scanner runs of a
    variant group: the four ranges with the default grid and a grid of 3, the
    second range once more with a bias of 2^40.  Cut short for the "run" group
    of the tables that match the 304 KiB run as one match (slow_run: the forest
    FIND resolves it serially, 0.3 to 1.5 s per scan on an MI355X): below the
    seam with the exit behind it, the whole run with both grids, and from the
    seam inside the run."""
    if group == "run" and tab.slow_run:
        return [(0, None, 0), (1, None, 0), (1, 3, 0), (2, None, 0)]
    return [(r, g, 0) for r in range(4) for g in (None, 3)] + [(1, None, 1 << 40)]


def scan_ranges(L, w):
    """The Scanner ranges of window w; a window that is not the last one stops
    64 bytes before its end (the window's own filler), where the oracle of the
    window alone and the buffer still read the same bytes."""
    S, top = L.seams[w], L.N if w == len(L.seams) - 1 else L.wend(w) - 64
    return [(L.wbase(w) + 1237, S - 5), (S - L.rhalf, S + L.rhalf), (S, top), (S + 1, top)]


# --- line references ---------------------------------------------------------

class Lines:
    """The line table of the whole buffer whose windows all hold `win`, from
    linesel_model.line_table(win) and the filler's period."""

    def __init__(self, L, win):
        self.L, self.win = L, win
        wb, we = linesel_model.line_table(win)
        assert win[-1] == 10
        begin, end, self.first = [], [], []
        pos = 0
        for w in range(len(L.seams)):
            k = (L.wbase(w) - pos) // L.P
            fb = pos + np.arange(k, dtype=np.int64) * L.P
            begin += [fb, wb + L.wbase(w)]
            end += [fb + L.P - 1, we + L.wbase(w)]
            self.first.append(sum(a.size for a in begin[:-1]))   # 0-based line of the window's first byte
            pos = L.wend(w)
        assert pos == L.N
        self.begin = np.concatenate(begin).astype(U64)
        self.end = np.concatenate(end).astype(U64)
        self.nwin = wb.size
        self.nl = np.flatnonzero(win == 10)

    @property
    def count(self):
        return self.begin.size

    def rel(self, starts, w):
        """The window-relative part of a sorted list of buffer offsets that lies in window w."""
        s = np.asarray(starts, U64)
        m = (s >= U64(self.L.wbase(w))) & (s < U64(self.L.wend(w)))
        return m, (s[m] - U64(self.L.wbase(w))).astype(np.int64)

    def touched(self, starts, lens=None):
        """bool per line of the buffer: linesel_model.touched on each window."""
        s = np.asarray(starts, U64)
        t = np.zeros(self.count, bool)
        seen = np.zeros(s.size, bool)
        for w in range(len(self.L.seams)):
            m, r = self.rel(s, w)
            seen |= m
            ln = None if lens is None else np.asarray(lens)[m]
            t[self.first[w]:self.first[w] + self.nwin] = linesel_model.touched(self.win, r, ln)
        assert seen.all(), "a match outside the windows"
        return t

    def records(self, pick):
        sel = np.flatnonzero(pick)
        return self.begin[sel], self.end[sel], (sel + 1).astype(U64)

    def select(self, starts, lens=None, invert=False):
        """ugpu_select_lines: (begin, end, lineno), lines."""
        t = self.touched(starts, lens)
        return self.records(~t if invert else t) + (self.count,)

    def select_bool(self, lists, clauses, invert=False, files=False):
        """ugpu_select_lines_bool: (begin, end, lineno), lines, whole; the
        formula is boolsel_model.formula over the folded literals."""
        lit = np.stack([self.touched(s, ln) for s, ln in lists])
        if files:
            whole = bool(boolsel_model.formula(lit.any(axis=1).reshape(-1, 1), clauses)[0])
            pick = lit.any(axis=0) if whole else np.zeros(self.count, bool)
        else:
            pick = boolsel_model.formula(lit, clauses)
            whole = None
        if invert:
            pick = ~pick
        if whole is None:
            whole = bool(pick.any())
        return self.records(pick) + (self.count, whole)

    def spans(self, lineno):
        q = np.asarray(lineno, U64)
        ok = (q >= 1) & (q <= self.count)
        idx = np.where(ok, q, 1).astype(np.int64) - 1
        return np.where(ok, self.begin[idx], FULL), np.where(ok, self.end[idx], FULL)

    def line_of(self, starts):
        """ugpu_lines: (newlines, matching_lines, d_line)."""
        s = np.asarray(starts, U64)
        line = np.zeros(s.size, U64)
        for w in range(len(self.L.seams)):
            m, r = self.rel(s, w)
            line[m] = (self.first[w] + 1 + np.searchsorted(self.nl, r, side="left")).astype(U64)
        assert (line > 0).all()
        newlines = int(np.count_nonzero(self.end < U64(self.L.N)))
        return newlines, int(np.unique(line).size), line

    def split(self, bounds, rec):
        """ugpu_split_matches for bounds that are, window by window, offsets
        inside that window (the first window's first bound to the last
        window's last): batch_model.split on each window, the segment between
        two windows being filler without a record."""
        nw = len(self.L.seams)
        assert len(bounds) == nw
        out = {k: [] for k in ("first", "digest", "dcap", "newlines", "mlines", "rel", "line")}
        base = 0
        for w in range(nw):
            m, r = self.rel(rec[0], w)
            b = np.asarray(bounds[w], U64) - U64(self.L.wbase(w))
            d = batch_model.split(self.win, b, r.astype(U64), rec[1][m], rec[2][m])
            out["first"].append(d["first"] + U64(base))
            for k in ("digest", "dcap", "newlines", "mlines"):
                out[k].append(d[k])
                if w + 1 < nw:   # the filler between this window's last bound and the next one's first
                    gap = (int(bounds[w + 1][0]) - int(bounds[w][-1])) // self.L.P
                    assert int(bounds[w][-1]) == self.L.wend(w) and int(bounds[w + 1][0]) == self.L.wbase(w + 1)
                    out[k].append(np.asarray([gap if k == "newlines" else 0], U64))
            out["rel"].append(d["rel"])
            out["line"].append(d["line"])
            base += int(m.sum())
        return {k: np.concatenate(v).astype(U64) for k, v in out.items()}


def seam_list(L, extra=()):
    """A hand-made sorted match list around every seam: matches that end on,
    start on and cross it (and the line ends the nl / crlf variants put there)."""
    st, ln = [], []
    for S in L.seams:
        for s, l in ((S - 40, 3), (S - 3, 2), (S - 1, 2), (S, 1), (S + 1, 3), (S + 30, 0)) + tuple(extra):
            st.append(s)
            ln.append(l)
    return np.asarray(st, U64), np.asarray(ln, U64)


# --- stream reference --------------------------------------------------------

def stream_chunk(n, period, plants):
    """A chunk of n bytes of filler (a '\\n' closing every period) with the
    byte strings `plants` = [(offset, bytes)] written into it."""
    chunk = np.full(n, F, np.uint8)
    chunk[period - 1::period] = 10
    for at, word in plants:
        assert 0 <= at and at + len(word) <= n
        chunk[at:at + len(word)] = np.frombuffer(word, np.uint8)
    return chunk


def stream_expected(tab, chunk, feeds, edge):
    """Records of `chunk` fed `feeds` times, from the oracle over two chunks:
    those that start before the last `edge` bytes of the first chunk, then the
    records of the following period (from there to `edge` bytes before the end
    of the second chunk) once per further chunk, moved by the chunk's length.
    The last `edge` bytes of a chunk must hold no complete match (they are the
    head of one that the next chunk finishes)."""
    n = chunk.size
    st, ln, cp = records(tab, np.concatenate([chunk, chunk]), 0)
    first = st < U64(n - edge)
    per = (st >= U64(n - edge)) & (st < U64(2 * n - edge))
    assert np.all((st + ln)[first] <= U64(n - edge))
    k = np.arange(feeds - 1, dtype=U64) * U64(n)
    return (np.concatenate([st[first], (st[per][None, :] + k[:, None]).reshape(-1)]),
            np.concatenate([ln[first], np.tile(ln[per], feeds - 1)]),
            np.concatenate([cp[first], np.tile(cp[per], feeds - 1)]))
