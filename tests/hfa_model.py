"""Pattern::match_hfa (lib/pattern.cpp:4757-4815) restated in plain Python over
the flattened automaton of ugrep_amd/csrc/hfa.hpp, with the behaviours of the
code as written:

  * the two visit sets alternate by level & 1 and are never cleared;
  * level 0 tests every entry;
  * an entry's offsets are tried in ascending order up to the first that
    fails; every offset that passes marks the entry's successors (so the first
    alone decides whether it propagates), and a dead entry's first passing
    offset ends the query with keep;
  * a level on which no entry passed all its offsets ends the query with skip.

The words: [magic, levels, entries, pairs, ranges, succs, states, flags],
level_first[17], entry_state[E], entry_dead[E], entry_pair[E+1],
entry_succ[E+1], pair_range[P+1], succ[S], range[R] (lo | hi << 16)."""
import numpy as np

MAGIC = 0x31414648
DEPTH, CHAIN = 16, 8


class Flat:
    """The arrays of the words (numpy views)."""

    def __init__(self, words):
        w = np.asarray(words, dtype=np.uint32).astype(np.int64)
        assert int(w[0]) == MAGIC
        self.levels, E, P, R, S, self.states, self.flags = (int(x) for x in w[1:8])
        self.p = 8

        def take(n):
            a = w[self.p:self.p + n]
            self.p += n
            return a
        self.level_first = take(DEPTH + 1)
        self.entry_state = take(E)
        self.entry_dead = take(E)
        self.entry_pair = take(E + 1)
        self.entry_succ = take(E + 1)
        self.pair_range = take(P + 1)
        self.succ = take(S)
        rng = take(R)
        self.lo, self.hi = rng & 0xFFFF, rng >> 16
        assert self.p == w.size


def pack(levels):
    """Words from a hand-written automaton: levels is a list (by level) of
    entries (state, dead, [per offset a list of (lo, hi)], [successors]); an
    entry of level l carries min(l, 7) + 1 offsets."""
    level_first, entry_state, entry_dead, entry_pair, entry_succ, pair_range, succ, rng = [], [], [], [], [], [], [], []
    for l, entries in enumerate(levels):
        level_first.append(len(entry_state))
        for state, dead, offsets, nxt in entries:
            assert len(offsets) == min(l, CHAIN - 1) + 1
            entry_state.append(state)
            entry_dead.append(int(dead))
            entry_pair.append(len(pair_range))
            entry_succ.append(len(succ))
            succ += [] if dead else list(nxt)
            for ranges in offsets:
                pair_range.append(len(rng))
                rng += [lo | (hi << 16) for lo, hi in ranges]
    E = len(entry_state)
    level_first += [E] * (DEPTH + 1 - len(level_first))
    entry_pair.append(len(pair_range))
    entry_succ.append(len(succ))
    pair_range.append(len(rng))
    states = max(entry_state + succ + [0]) + 1
    head = [MAGIC, len(levels), E, len(pair_range) - 1, len(rng), len(succ), states, 0]
    return np.array(head + level_first + entry_state + entry_dead + entry_pair + entry_succ + pair_range + succ + rng,
                    dtype=np.uint32)


def match(words, table):
    """True: keep the file.  words: the automaton's words or a Flat; empty: no
    automaton, keep."""
    if not isinstance(words, Flat):
        if len(words) == 0:
            return True
        words = Flat(words)
    f = words
    t = np.frombuffer(bytes(table), np.uint8) if not isinstance(table, np.ndarray) else table
    size = t.size
    assert size and size & (size - 1) == 0
    # count[k][i]: the slots before i (of the table laid out twice, so that a walk
    # that wraps is one span) in which bit k is clear
    count = [np.concatenate([[0], np.cumsum(np.tile((t & (1 << k)) == 0, 2))]) for k in range(8)]
    visit = [set(), set()]
    for level in range(DEPTH):
        cur, nxt = visit[level & 1], visit[(level + 1) & 1]
        any_all = False
        for e in range(int(f.level_first[level]), int(f.level_first[level + 1])):
            if level and int(f.entry_state[e]) not in cur:
                continue
            p0, p1 = int(f.entry_pair[e]), int(f.entry_pair[e + 1])
            passed_all = True
            for p in range(p0, p1):
                c = count[p1 - 1 - p]  # bit level - offset
                r0, r1 = int(f.pair_range[p]), int(f.pair_range[p + 1])
                lo = f.lo[r0:r1]
                n = np.minimum(f.hi[r0:r1] - lo + 1, size)  # a range as long as the table meets every slot
                a = lo & (size - 1)
                if not (c[a + n] > c[a]).any():
                    passed_all = False
                    break
                if f.entry_dead[e]:
                    return True
                nxt.update(f.succ[int(f.entry_succ[e]):int(f.entry_succ[e + 1])].tolist())
            any_all = any_all or passed_all
        if not any_all:
            return False
    return True


def keep_record(words, header, table, ignore_binary=False, decompress=False):
    """The decision per record (src/ugrep.cpp:10060-10099)."""
    if not isinstance(words, Flat) and len(words) == 0:
        return True  # no automaton: the index is off, whatever the header says (src/ugrep.cpp:8931)
    if (header & 0x80 and ignore_binary) or (header & 0x60 and not decompress):
        return False
    return match(words, table) if header & 0x1F else bool(header & 0x80)


# ---- the corpus and the patterns of tests/golden/hfa_cases.json

SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 40, 64, 100, 200, 400, 800, 1500, 3000, 6000, 12000, 25000, 50000, 70000, 100000,
         200000)


def corpus():
    """The files as specifications: name, index_model.gen_input arguments and the bytes appended."""
    out = []
    for i, n in enumerate(SIZES):
        tail = " needle%02d zq%dx\n" % (i, i) if n >= 40 else ""
        if n == 400:
            tail += "abcbcd 2024 antique record\n"
        out.append({"name": "w%02d_%d.txt" % (i, n), "gen": ["words", n, 100 + i], "append": tail})
    out.append({"name": "ascii.txt", "gen": ["ascii", 5000, 1], "append": ""})
    out.append({"name": "low.txt", "gen": ["low", 5000, 2], "append": ""})
    out.append({"name": "utf8.txt", "gen": ["utf8", 5000, 3], "append": ""})
    out.append({"name": "random.bin", "gen": ["random", 20000, 4], "append": ""})
    out.append({"name": "empty.txt", "gen": ["words", 0, 0], "append": ""})
    out.append({"name": "a777.txt", "gen": ["repeat", 777, 0x61], "append": ""})
    return out


def corpus_bytes(spec):
    import index_model as im
    return im.gen_input(*spec["gen"]) + spec["append"].encode()


def word_set(n=100, seed=7):
    """n distinct seeded lower-case words of 4 to 8 letters, and two of index_model.WORDS."""
    rs = np.random.RandomState(seed)
    words = ["kernel", "bloom"]
    while len(words) < n:
        w = "".join(chr(0x61 + c) for c in rs.randint(0, 26, rs.randint(4, 9)))
        if w not in words:
            words.append(w)
    return words


def patterns():
    lit26 = "abcdefghijklmnopqrstuvwxyz"
    plain = ["a", "of", "the that", "with be b", "record store bin", "record store bina", lit26,  # lengths 1 2 8 9 16 17 26
             "kernel", "zyzzyva", "needle07", "needle0[1-3]", "needle(07|19)x?", "hash|bloom",
             "the|thereof", "ab|abcd", "a(bc)*d", "n(ee)+dle", "[a-z]+que",
             "[a-z]{3}ord", "recor[a-z]", "tab.e", "zq[0-9]+x", "[0-9]{4}",
             "\\w+", "[^a-z ]{2}", "é+", "α|€", "[\\x80-\\xff]e", "a*", "kernel\\b", "^index",
             "|".join(word_set())]
    assert [len(p) for p in plain[:7]] == [1, 2, 8, 9, 16, 17, 26]
    out = [{"pattern": p, "args": []} for p in plain]
    out.append({"pattern": "kernel", "args": ["-i"]})
    out.append({"pattern": "a(bc)*d", "args": ["-F"]})
    return out
