"""Models of the column semantics (include/ugpu.h, ugpu_columns), shared by
tests/test_columns_host.py and tests/test_columns.py.

direct()      the reference's fold, byte by byte (AbstractMatcher::columno(),
              absmatcher.h:795-816), at every position 0..len;
direct_np()   the same in numpy (a Python step per tab only), for large inputs;
stitched()    the shape of the device call: a summary per byte range (newline
              count, last newline, the column function of its tail), the host
              stitch, and an assign pass that applies the function of the
              range's bytes before each position to the range's incoming
              column, with the input cut into ranges of any size.

A column function is (kind, a, b): ADD k -> k + a; TAB k -> ((k + a) | (T-1)) +
1 + b; CONST k -> a (the range holds a newline)."""
import numpy as np

ADD, TAB, CONST = 0, 1, 2
FULL = 0xFFFFFFFFFFFFFFFF


def direct(data, tab=8):
    """(col, bol, line) lists of len + 1 entries: the fold itself."""
    data = bytes(bytearray(np.asarray(data, np.uint8)))
    col, bol, line = [0] * (len(data) + 1), [0] * (len(data) + 1), [1] * (len(data) + 1)
    k, b, ln = 0, 0, 1
    for p, c in enumerate(data):
        if c == 10:
            k, b, ln = 0, p + 1, ln + 1
        elif c == 9:
            k += 1 + (~k & (tab - 1))
        else:
            k += (c & 0xC0) != 0x80
        col[p + 1], bol[p + 1], line[p + 1] = k, b, ln
    return col, bol, line


def direct_np(data, tab=8, k0=0):
    """(col, bol, line) int64 arrays of len + 1 entries; k0 is the column at
    position 0 (a line that began before the data)."""
    data = np.asarray(data, np.uint8)
    n = data.size
    isnl, istab = data == 10, data == 9
    plain = ((data & 0xC0) != 0x80) & ~istab
    cs = np.concatenate([[0], np.cumsum(plain)]).astype(np.int64)    # plain bytes in [0, p)
    nlpos = np.flatnonzero(isnl).astype(np.int64)
    p = np.arange(n + 1, dtype=np.int64)
    nbefore = np.searchsorted(nlpos, p, side="left")                 # newlines in [0, p)
    bol = np.where(nbefore > 0, nlpos[np.maximum(nbefore, 1) - 1] + 1 if nlpos.size else 0, 0)
    # anchors: position 0 and the position behind each newline or tab, with the column there
    anch = np.flatnonzero(isnl | istab)
    apos = np.concatenate([[0], anch + 1]).astype(np.int64)
    aval = np.zeros(apos.size, np.int64)
    aval[0] = k0
    for i in np.flatnonzero(istab[anch]).tolist():                  # anchor i + 1 is behind a tab
        k = int(aval[i]) + int(cs[anch[i]] - cs[apos[i]])
        aval[i + 1] = (k | (tab - 1)) + 1
    ai = np.searchsorted(apos, p, side="right") - 1                  # the last anchor at or before p
    col = aval[ai] + cs[p] - cs[apos[ai]]
    return col, bol.astype(np.int64), (nbefore + 1).astype(np.int64)


def expected(data, pos, tab=8):
    """(col, bol, line) uint64 arrays for a position list; UINT64_MAX past len."""
    data = np.asarray(data, np.uint8)
    col, bol, line = direct_np(data, tab)
    pos = np.asarray(pos, np.uint64)
    ok = pos <= np.uint64(data.size)
    at = np.where(ok, pos, 0).astype(np.int64)
    full = np.uint64(FULL)
    return tuple(np.where(ok, a[at].astype(np.uint64), full) for a in (col, bol, line))


def compose(f, g, tab):
    """first f, then g"""
    if g[0] == CONST:
        return g
    tm = tab - 1
    if g[0] == ADD:
        if f[0] == TAB:
            return (TAB, f[1], f[2] + g[1])
        return (f[0], f[1] + g[1], 0)
    if f[0] == ADD:
        return (TAB, f[1] + g[1], g[2])
    if f[0] == TAB:
        return (TAB, f[1], ((f[2] + g[1]) | tm) + 1 + g[2])
    return (CONST, ((f[1] + g[1]) | tm) + 1 + g[2], 0)


def apply(f, k, tab):
    if f[0] == CONST:
        return f[1]
    if f[0] == TAB:
        return ((k + f[1]) | (tab - 1)) + 1 + f[2]
    return k + f[1]


def byte_fn(c):
    if c == 10:
        return (CONST, 0, 0)
    if c == 9:
        return (TAB, 0, 0)
    return (ADD, int((c & 0xC0) != 0x80), 0)


def stitched(data, tab=8, per=4096):
    """(col, bol, line) lists of len + 1 entries through summary, stitch and assign."""
    data = bytes(bytearray(np.asarray(data, np.uint8)))
    n = len(data)
    ranges = [(lo, min(lo + per, n)) for lo in range(0, n, per)] or [(0, 0)]
    summ = []
    for lo, hi in ranges:                       # summary pass
        f, cnt, last = (ADD, 0, 0), 0, 0
        for p in range(lo, hi):
            f = compose(f, byte_fn(data[p]), tab)
            if data[p] == 10:
                cnt, last = cnt + 1, p + 1
        summ.append((cnt, last, f))
    state, nl, b, k = [], 0, 0, 0               # stitch
    for cnt, last, f in summ:
        state.append((nl, b, k))
        nl, b, k = nl + cnt, (last or b), apply(f, k, tab)
    col, bol, line = [0] * (n + 1), [0] * (n + 1), [1] * (n + 1)
    for (lo, hi), (nl0, b0, k0) in zip(ranges, state):   # assign pass
        f, b, ln = (ADD, 0, 0), b0, 1 + nl0
        for p in range(lo, hi):
            col[p], bol[p], line[p] = apply(f, k0, tab), b, ln
            f = compose(f, byte_fn(data[p]), tab)
            if data[p] == 10:
                b, ln = p + 1, ln + 1
        if hi == n:
            col[n], bol[n], line[n] = apply(f, k0, tab), b, ln
    return col, bol, line
