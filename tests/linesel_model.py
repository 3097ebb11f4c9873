"""numpy model of the line-record semantics (include/ugpu.h, ugpu_select_lines
and ugpu_line_spans), shared by tests/test_linesel_host.py and
tests/test_linesel.py."""
import numpy as np


def line_table(data):
    """(begin, end) int64 arrays of every line of `data` (uint8 array): end is
    the offset of the line's '\\n', or len for an unterminated last line."""
    data = np.asarray(data, np.uint8)
    nl = np.flatnonzero(data == 10).astype(np.int64)
    end = nl
    if len(data) and (len(nl) == 0 or nl[-1] != len(data) - 1):
        end = np.append(nl, len(data))
    begin = np.append(0, end[:-1] + 1)[:len(end)].astype(np.int64)
    return begin, end.astype(np.int64)


def touched(data, starts, lens=None):
    """bool per line: some match (s, l) with s < len touches it."""
    data = np.asarray(data, np.uint8)
    n = len(data)
    begin, end = line_table(data)
    s = np.asarray(starts, np.int64).reshape(-1)
    ln = np.zeros(len(s), np.int64) if lens is None else np.asarray(lens, np.int64).reshape(-1)
    keep = s < n
    s, ln = s[keep], ln[keep]
    last = np.minimum(np.maximum(s, s + ln - 1), n - 1)
    nl = np.flatnonzero(data == 10)
    a = np.searchsorted(nl, s, side="left")     # newlines before the byte: its 0-based line
    b = np.searchsorted(nl, last, side="left")
    d = np.zeros(len(begin) + 1, np.int64)
    np.add.at(d, a, 1)
    np.add.at(d, b + 1, -1)
    return np.cumsum(d)[:len(begin)] > 0


def select(data, starts, lens=None, invert=False):
    """(begin, end, lineno) uint64 arrays of the selected lines, and the line count."""
    begin, end = line_table(data)
    t = touched(data, starts, lens)
    sel = np.flatnonzero(~t if invert else t)
    return begin[sel].astype(np.uint64), end[sel].astype(np.uint64), (sel + 1).astype(np.uint64), len(begin)


def context_sets(selected, nlines, before, after):
    """Brute force: (sorted printed line numbers, kinds) from a per-line mask,
    one shifted copy of the selection per context distance."""
    sel = np.asarray(selected, np.int64).reshape(-1)
    chosen = np.zeros(nlines + 2, bool)
    out = np.zeros(nlines + 2, bool)
    chosen[sel] = True
    for d in range(-before, after + 1):
        k = sel + d
        out[k[(k >= 1) & (k <= nlines)]] = True
    lineno = np.flatnonzero(out)
    return lineno.tolist(), chosen[lineno].astype(int).tolist()


def grep(data, starts, lens, invert=False, before=0, after=0):
    """[(lineno, kind)] and the spans the CLI prints, from the model alone."""
    begin, end = line_table(data)
    _, _, sel, nlines = select(data, starts, lens, invert)
    lineno, kind = context_sets(sel, nlines, before, after)
    idx = np.asarray(lineno, np.int64) - 1
    return lineno, kind, begin[idx], end[idx]


def spans(data, lineno):
    begin, end = line_table(data)
    q = np.asarray(lineno, np.uint64)
    ok = (q >= 1) & (q <= len(begin))
    idx = np.where(ok, q, 1).astype(np.int64) - 1
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    if len(begin) == 0:
        return np.full(len(q), full), np.full(len(q), full)
    return (np.where(ok, begin[idx].astype(np.uint64), full), np.where(ok, end[idx].astype(np.uint64), full))
