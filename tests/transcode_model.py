"""Models of the input conversions (include/ugpu.h, ugpu_transcode), shared by
tests/test_transcode_host.py and tests/test_transcode.py.

direct()    the reference's loops, unit by unit (Input::file_get,
            lib/input.cpp:748-1023, one call with an unbounded n);
stitched()  the shape of the device call, vectorised: per byte range of `per`
            bytes the output length for both incoming bits and the range's
            carry function, the host stitch (offsets and incoming bits), and a
            write pass per range that knows only its own bytes, the unit
            behind them, its offset and its incoming bit;
detect_bom(), bound()  the tables of ugpu_detect_bom and ugpu_transcode_bound.

The carry of UTF-16: a high surrogate consumes the unit behind it.  A range
maps the bit "my first unit is consumed" to the same bit of the unit behind
the range; the function is kept as its two values (f[0], f[1])."""
import json
import os

import numpy as np

PLAIN, UTF8, UTF16BE, UTF16LE, UTF32BE, UTF32LE, LATIN1, PAGE, NULL_DATA = range(9)
NONCHAR = b"\xf8\x88\x80\x80\x80"
ENCS = (UTF16BE, UTF16LE, UTF32BE, UTF32LE, LATIN1, PAGE, NULL_DATA)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = {"utf16be": UTF16BE, "utf16le": UTF16LE, "utf32be": UTF32BE, "utf32le": UTF32LE, "latin1": LATIN1,
         "page": PAGE, "null_data": NULL_DATA}


def utf8(c):
    """reflex::utf8(int, char*), include/reflex/utf8.h:76-135"""
    if c < 0x80:
        return bytes([c & 0xFF])
    if c > 0x10FFFF:
        return NONCHAR
    if c < 0x800:
        return bytes([0xC0 | (c >> 6), 0x80 | (c & 0x3F)])
    if c < 0x10000:
        return bytes([0xE0 | (c >> 12), 0x80 | ((c >> 6) & 0x3F), 0x80 | (c & 0x3F)])
    return bytes([0xF0 | (c >> 18), 0x80 | ((c >> 12) & 0x3F), 0x80 | ((c >> 6) & 0x3F), 0x80 | (c & 0x3F)])


def direct(data, enc, page=None):
    data = bytes(bytearray(data))
    out = bytearray()
    if enc in (UTF16BE, UTF16LE):
        order = "big" if enc == UTF16BE else "little"
        i, n = 0, len(data)
        while i + 2 <= n:
            c = int.from_bytes(data[i:i + 2], order)
            i += 2
            if c < 0x80:
                out.append(c)
                continue
            if 0xD800 <= c < 0xE000:
                if c < 0xDC00 and i + 2 <= n:
                    d = int.from_bytes(data[i:i + 2], order)
                    i += 2                       # consumed whatever it is
                    c = 0x10000 + ((c - 0xD800) << 10) + (d - 0xDC00) if (d & 0xFC00) == 0xDC00 else 0x200000
                elif c < 0xDC00:
                    i = n                        # fewer than two bytes behind it: the input ends
                    c = 0x200000
                else:
                    c = 0x200000
            out += utf8(c)
    elif enc in (UTF32BE, UTF32LE):
        order = "big" if enc == UTF32BE else "little"
        for i in range(0, len(data) - 3, 4):
            c = int.from_bytes(data[i:i + 4], order, signed=True)
            out += bytes([c & 0xFF]) if c < 0x80 else utf8(c)
    elif enc == LATIN1:
        for b in data:
            out += bytes([b]) if b < 0x80 else utf8(b)
    elif enc == PAGE:
        for b in data:
            c = int(page[b])
            out += bytes([c]) if c < 0x80 else utf8(c)
    elif enc == NULL_DATA:
        out += data.translate(bytes([10 if b == 0 else 0 if b == 10 else b for b in range(256)]))
    else:
        raise ValueError(enc)
    return bytes(out)


def detect_bom(head, length=None):
    head = bytes(head[:4])
    n = len(head) if length is None else length
    head = head[:min(n, 4)]
    if n >= 4 and head == b"\x00\x00\xfe\xff":
        return UTF32BE, 4
    if head[:2] == b"\xfe\xff":
        return UTF16BE, 2
    if n >= 4 and head == b"\xff\xfe\x00\x00":
        return UTF32LE, 4
    if n >= 4 and head[:2] == b"\xff\xfe":
        return UTF16LE, 2
    if head[:3] == b"\xef\xbb\xbf":
        return UTF8, 3
    return PLAIN, 0


def bound(enc, nbytes):
    return {UTF16BE: nbytes // 2 * 5, UTF16LE: nbytes // 2 * 5, UTF32BE: nbytes // 4 * 5, UTF32LE: nbytes // 4 * 5,
            LATIN1: nbytes * 2, PAGE: nbytes * 3, NULL_DATA: nbytes}[enc]


# ---- the vectorised, stitched model

def _units(data, enc):
    """(code units as int64, bytes per unit)"""
    data = np.frombuffer(bytes(bytearray(data)), np.uint8)
    if enc in (UTF16BE, UTF16LE):
        m = data.size // 2
        return data[:2 * m].view(">u2" if enc == UTF16BE else "<u2").astype(np.int64), 2
    if enc in (UTF32BE, UTF32LE):
        m = data.size // 4
        return data[:4 * m].view(">i4" if enc == UTF32BE else "<i4").astype(np.int64), 4
    return data.astype(np.int64), 1


def _encode(cp, raw):
    """UTF-8 of the code points cp (utf8() above; raw: the low byte as it is):
    (lengths, bytes as an (n, 5) array of which the first lengths[i] count)."""
    cp = np.asarray(cp, np.int64)
    ln = np.where(raw | (cp < 0x80), 1, np.where(cp < 0x800, 2, np.where(cp < 0x10000, 3, np.where(cp <= 0x10FFFF, 4, 5))))
    b = np.zeros((cp.size, 5), np.uint8)
    one, two, three, four, five = (ln == k for k in (1, 2, 3, 4, 5))
    b[one, 0] = cp[one] & 0xFF
    b[two, 0] = 0xC0 | (cp[two] >> 6)
    b[two, 1] = 0x80 | (cp[two] & 0x3F)
    b[three, 0] = 0xE0 | (cp[three] >> 12)
    b[three, 1] = 0x80 | ((cp[three] >> 6) & 0x3F)
    b[three, 2] = 0x80 | (cp[three] & 0x3F)
    b[four, 0] = 0xF0 | (cp[four] >> 18)
    b[four, 1] = 0x80 | ((cp[four] >> 12) & 0x3F)
    b[four, 2] = 0x80 | ((cp[four] >> 6) & 0x3F)
    b[four, 3] = 0x80 | (cp[four] & 0x3F)
    b[five] = np.frombuffer(NONCHAR, np.uint8)
    return ln, b


def _seconds(h, c):
    """The consumed units of a stretch whose H units are h (bool array), with
    the incoming bit c: an array of h.size + 1 bools, the last the outgoing bit."""
    n = h.size
    s = np.zeros(n + 1, bool)
    s[0] = bool(c)
    if n == 0:
        return s
    h = h.copy()
    if c:
        h[0] = False                             # a consumed unit takes part in no run
    idx = np.arange(n)
    start = h & ~np.concatenate([[False], h[:-1]])
    run0 = np.maximum.accumulate(np.where(start, idx, -1))     # the begin of the run a unit is in
    s[1:] |= h & ((idx - run0) % 2 == 0)         # the unit behind an H unit at an even place of its run
    return s


def _range_units(u, nxt, enc, page, c):
    """(code points, raw flags, emitted flags, outgoing bit) of a range's units
    u, nxt the unit behind them (None at the end of the input), c the incoming bit."""
    if enc in (UTF16BE, UTF16LE):
        h = (u & 0xFC00) == 0xD800
        low = (u & 0xFC00) == 0xDC00
        s = _seconds(h, c)
        follow = np.concatenate([u[1:], [nxt if nxt is not None else 0]]) if u.size else u
        pair = h & ((follow & 0xFC00) == 0xDC00)
        if u.size and nxt is None:
            pair[-1] = False
        cp = np.where(pair, 0x10000 + ((u - 0xD800) << 10) + (follow - 0xDC00), np.where(h | low, 0x200000, u))
        return cp, np.zeros(u.size, bool), ~s[:-1], int(s[-1])
    if enc in (UTF32BE, UTF32LE):
        raw = u < 0x80
        return np.where(raw, u & 0xFF, u), raw, np.ones(u.size, bool), 0
    if enc == LATIN1:
        return u, np.zeros(u.size, bool), np.ones(u.size, bool), 0
    if enc == PAGE:
        return np.asarray(page, np.int64)[u], np.zeros(u.size, bool), np.ones(u.size, bool), 0
    return np.where(u == 0, 10, np.where(u == 10, 0, u)), np.ones(u.size, bool), np.ones(u.size, bool), 0


def stitched(data, enc, page=None, per=4096):
    """The conversion through range summaries, the stitch and a write pass per
    range; `per` (a multiple of the unit size) is the bytes per range."""
    u, w = _units(data, enc)
    assert per % w == 0
    step = per // w
    ranges = [(lo, min(lo + step, u.size)) for lo in range(0, u.size, step)] or [(0, 0)]

    def part(lo, hi, c):
        nxt = int(u[hi]) if hi < u.size else None
        cp, raw, emit, cout = _range_units(u[lo:hi], nxt, enc, page, c)
        ln, b = _encode(cp[emit], raw[emit])
        return ln, b, cout

    summ = []
    for lo, hi in ranges:                        # summary pass: both incoming bits
        l0, _, o0 = part(lo, hi, 0)
        l1, _, o1 = part(lo, hi, 1)
        summ.append((int(l0.sum()), int(l1.sum()), (o0, o1)))
    state, off, c = [], 0, 0                     # stitch
    for n0, n1, f in summ:
        state.append((off, c))
        off, c = off + (n1 if c else n0), f[c]
    out = np.zeros(off, np.uint8)
    for (lo, hi), (o, cin) in zip(ranges, state):   # write pass
        ln, b, _ = part(lo, hi, cin)
        keep = np.arange(5)[None, :] < ln[:, None]
        seg = b[keep]
        out[o:o + seg.size] = seg
    return out.tobytes()


# ---- the fixture and random inputs of both test files

def load_cases():
    """[(name, input bytes, enc, skip, page, recorded CLI output)], the pages, the whole fixture"""
    with open(os.path.join(GOLDEN, "transcode_cases.json")) as f:
        g = json.load(f)
    blob = open(os.path.join(GOLDEN, g["inputs"]), "rb").read()
    out = []
    for c in g["cases"]:
        if "file" in c:
            data = open(os.path.join(GOLDEN, c["file"]), "rb").read()
        else:
            data = blob[c["input"][0]:c["input"][0] + c["input"][1]]
        page = None
        if c["enc"] == "bom":
            enc, skip = detect_bom(data[:4], len(data))
        elif c["enc"].startswith("page:"):
            enc, skip, page = PAGE, 0, g["pages"][c["enc"][5:]]
        else:
            enc, skip = NAMES[c["enc"]], 0
        out.append((c["name"], data, enc, skip, page, bytes.fromhex(c["out"])))
    return out, g


def printed(stream):
    """what the CLI prints for a converted stream: its lines, the last one ended"""
    return stream if not stream or stream.endswith(b"\n") else stream + b"\n"


def random_input(rng, enc, n):
    """n bytes; UTF-16 draws about 30 % high and 30 % low surrogates"""
    if enc in (UTF16BE, UTF16LE):
        m = (n + 1) // 2
        kind = rng.random(m)
        u = np.where(kind < 0.3, rng.integers(0xD800, 0xDC00, m),
                     np.where(kind < 0.6, rng.integers(0xDC00, 0xE000, m),
                              np.where(kind < 0.8, rng.integers(0, 0x100, m), rng.integers(0, 0x10000, m))))
        return u.astype(">u2" if enc == UTF16BE else "<u2").tobytes()[:n]
    if enc in (UTF32BE, UTF32LE):
        m = (n + 3) // 4
        kind = rng.random(m)
        u = np.where(kind < 0.4, rng.integers(0, 0x100, m),
                     np.where(kind < 0.7, rng.integers(0, 0x11100, m),
                              np.where(kind < 0.9, rng.integers(0, 0x120000, m), rng.integers(0, 1 << 32, m))))
        return u.astype(">u4" if enc == UTF32BE else "<u4").tobytes()[:n]
    pool = np.concatenate([np.arange(256), [0, 10, 10, 0x41, 0x7F, 0x80, 0xFF] * 8])
    return pool[rng.integers(0, pool.size, n)].astype(np.uint8).tobytes()


def random_page(rng):
    page = rng.integers(0, 0x10000, 256)
    page[:0x80:3] = np.arange(0x80)[::3]
    return page.tolist()
