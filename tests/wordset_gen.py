"""Seeded word sets and texts for the n-gram kernel's tests (kernel 7,
ugrep_amd/csrc/ngram_kernel.hip): shared by tests/golden/make_wordset_golden.py,
tests/test_wordset_host.py and tests/test_wordset.py, so that the golden file
stores seeds and totals instead of the larger sets.

Words are syllable words of 4-12 bytes (lengths skewed short, as in text), in
one seeded sequence: words(n) is a prefix of words(m) for n < m.  A few words
with UTF-8 letters follow the first ones."""
import random

import numpy as np

SEED = 20261020
_SYL = [c + v for c in "bcdfghjklmnprstvwz" for v in "aeiou"] + ["st", "nd", "ch", "th", "ing", "er", "an", "or"]
UTF8_WORDS = ["café", "naïve", "über", "straße", "中文字", "слово"]


def words(n, seed=SEED, utf8=True):
    """The first n words of the seeded sequence (str, unique, unsorted)."""
    r = random.Random(seed)
    out, seen = [], set()
    while len(out) < n:
        if utf8 and len(out) in (7, 19, 31, 43, 55, 67) and len(out) // 12 < len(UTF8_WORDS):
            w = UTF8_WORDS[len(out) // 12]
        else:
            k = 4 + int(9 * r.random() ** 2)  # 4..12, short words more often
            w = ""
            while len(w) < k:
                w += r.choice(_SYL)
            w = w[:k]
        if w not in seen and 4 <= len(w.encode()) <= 12:
            seen.add(w)
            out.append(w)
    return out


def regex(ws):
    """The alternation of the words (none holds a regex metacharacter)."""
    return "|".join(ws)


def edge_text(ws):
    """A small text around the words of a set: whole words between every kind
    of separator, words glued together, prefixes cut short, words inside longer
    words, other case, UTF-8 neighbours, and a word at the very end."""
    r = random.Random(SEED + 1)
    pick = [ws[i] for i in range(0, len(ws), max(1, len(ws) // 40))]
    parts = []
    for i, w in enumerate(pick):
        sep = [" ", "\n", ",", "_", "-", "1", "é", "", "x", "\t"][i % 10]
        parts.append(w + sep)
        if i % 3 == 0:
            parts.append(w[:-1] + " ")           # cut short
        if i % 4 == 0:
            parts.append(w + pick[(i + 1) % len(pick)] + " ")  # glued
        if i % 5 == 0:
            parts.append("q" + w + "q ")          # inside a longer word
        if i % 6 == 0:
            parts.append(w.upper() + " " + w.capitalize() + " ")
        if i % 7 == 0:
            parts.append(w[:3] + w + " ")         # its own prefix before it
        if i % 8 == 0:
            parts.append(r.choice(_SYL) * 3 + " ")
    parts.append("\n\n" + pick[0] + " last " + pick[-1])
    return "".join(parts).encode("utf-8")


def plant(buf, ws, every=997, seed=SEED + 2):
    """A copy of the uint8 array with words of the set written over it about
    every `every` bytes (half of them between spaces, some right after one
    another, some cut by the end)."""
    out = np.array(buf, dtype=np.uint8, copy=True)
    r = random.Random(seed)
    p = r.randrange(every)
    while p < len(out):
        w = np.frombuffer(r.choice(ws).encode("utf-8"), np.uint8)
        n = min(len(w), len(out) - p)
        out[p:p + n] = w[:n]
        if r.random() < 0.5:  # a whole word (option W)
            out[max(p - 1, 0)] = 32
            out[min(p + n, len(out) - 1)] = 32
        p += n + (0 if r.random() < 0.1 else r.randrange(1, 2 * every))
    return out


TILE = 4096  # the kernel's wave-tile


def tile_edge_buffers(ws, ngram=4, size=64 << 10):
    """[(name, uint8 array)]: one buffer per offset d in 0 .. ngram + 1, with a
    word of the set starting d bytes before every 4 KiB tile edge (so that it
    straddles the edge, and the n-gram windows of its first bytes do), over
    corpus text; every other word stands between spaces.  The last buffer ends
    in a whole word, the one before in a word cut off by the end."""
    from oracle_lib import gen
    long_ws = [w for w in ws if len(w.encode("utf-8")) >= ngram + 3]
    out = []
    for d in range(ngram + 2):
        buf = np.array(gen(1, 11 + d, 0, size), dtype=np.uint8, copy=True)
        for t in range(1, size // TILE):
            w = np.frombuffer(long_ws[(7 * t + d) % len(long_ws)].encode("utf-8"), np.uint8)
            p = t * TILE - d
            buf[p:p + len(w)] = w
            if t % 2 == 0:
                buf[p - 1] = buf[p + len(w)] = 32
        w = np.frombuffer(long_ws[d].encode("utf-8"), np.uint8)
        if d == ngram + 1:
            buf[size - len(w) - 1] = 32
            buf[size - len(w):] = w            # ends at the last byte
        elif d == ngram:
            buf[size - len(w) + 2 - 1] = 32
            buf[size - len(w) + 2:] = w[:-2]   # cut off by the end
        out.append(("edge_d%d" % d, buf))
    return out


def child_inputs(which):
    """(words in the set, [(name, buffer)]) of tests/wordset_child.py runs."""
    from oracle_lib import gen
    ws = words(300)
    if which == "edges":
        return 300, tile_edge_buffers(ws)
    if which == "corpus":
        return 300, tile_edge_buffers(ws)[:2] + [("gen1_1m", plant(gen(1, 5, 0, 1 << 20), ws))]
    raise ValueError(which)
