"""Layouts of tests/test_open_walks.py: inputs whose sparse_kernel waves end in
open walks that fix_kernel's R1 cannot resolve, so that R1b (coop_continue,
one wave per walk) has to.

A layout is a filler buffer (`12 \\n`: no candidate of the patterns used) with
plants.  A plant in record b is an `x`, d bytes before the end E of the
record's byte range, followed by L letters without `x` and then a byte that
ends the walk.  With L >= d + kOpenSlack + kOpenConvBudget + 1 the walk of the
`x` is alive where sparse_kernel stops it (E + kOpenSlack) and still alive,
with no other walk to converge with, where R1 gives up (E + kOpenSlack +
kOpenConvBudget): R1b walks the rest.  Where the `y` (an accept) lie is the
case's business.

The record ranges are the ones engine.hip geometry() deals for a 16-byte
aligned buffer scanned from 0 with UGPU_MAX_GRID=grid: tiles of kWaveTile
bytes, tpr = ceil(nt / min(nt, grid)) tiles a record.  The CPU test
tests/test_open_walks_host.py restates geometry() in full and R1 in Python and
checks, for every layout, the number of walks it leaves to R1b (`k`).
"""
import functools

import numpy as np

TILE = 4096              # kWaveTile
SLACK = 256              # kOpenSlack
CONV = 4096              # kOpenConvBudget
COOP_MAX = 256           # kOpenCoopMax
COOP_BUDGET = 64 << 20   # kOpenCoopBudget
FILL = b"12 \n"
LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwz", np.uint8)   # [a-wz]
D = (1, 17, 100, 255)

RX = "x[a-z]*y"
RX2 = "x[a-z]*y|x[a-z]*Z"      # two accept indices: Z ends a walk with an accept of its own
RX5 = "x([a-z]{5})*y"          # a letter loop of period 5: coop_continue's 4-byte guesses go wrong


def min_letters(d):
    """Letters after an `x` d bytes before a range end that keep its walk alive past R1."""
    return d + SLACK + CONV + 1


class Plant:
    def __init__(self, rec, x, die, end):
        self.rec, self.x, self.die, self.end = rec, x, die, end   # die: the first byte after the letters

    @property
    def r1_end(self):
        """Where R1 gives the walk up."""
        return self.end + SLACK + CONV


class Layout:
    """n bytes scanned as [0, n) with UGPU_MAX_GRID=grid; `tail` more bytes
    behind them (a readable end before the buffer's)."""

    def __init__(self, name, rx, n, grid, seed, tail=0):
        self.name, self.rx, self.n, self.grid, self.tail = name, rx, n, grid, tail
        nt = -(-n // TILE)
        self.tpr = -(-nt // min(nt, grid))
        self.rec = self.tpr * TILE
        self.nrec = -(-nt // self.tpr)
        self.host = np.frombuffer(FILL * ((n + tail) // len(FILL) + 1), np.uint8)[:n + tail].copy()
        self.rng = np.random.default_rng(seed)
        self.plants = []
        self.k = 0            # open walks R1 leaves unresolved
        self.forest = False   # whether the scan has to fall back to the forest FIND

    def range_start(self, b):
        return min(b * self.rec, self.n)

    def range_end(self, b):
        return min((b + 1) * self.rec, self.n)

    def letters(self, a, z):
        self.host[a:z] = LETTERS[self.rng.integers(0, LETTERS.size, z - a, dtype=np.uint8)]

    def used(self):
        return self.plants[-1].die if self.plants else -1

    def next_record(self):
        """The first record whose plant (any d) starts behind everything planted so far."""
        b = (self.used() + max(D)) // self.rec
        return b + 1 if self.range_end(b) - max(D) <= self.used() else b

    def plant(self, b, d, L, ys=(), kill=b" "):
        assert 0 <= b < self.nrec - 1, "the last record's walks are never open"
        end = self.range_end(b)
        x, die = end - d, end - d + 1 + L
        assert x > self.used(), "plants overlap"
        assert L >= min_letters(d) and die <= self.n + self.tail
        self.host[x] = ord("x")
        self.letters(x + 1, die)
        if die < self.n + self.tail:
            self.host[die] = ord(kill)
        for p in ys:
            assert x < p < die
            self.host[p] = ord("y")
        self.plants.append(Plant(b, x, die, end))
        return self.plants[-1]

    def freeze(self):
        self.host.setflags(write=False)
        return self


def wave_split(K):
    """K unresolved walks of 4.5 KiB to 200 KiB in shuffled order (the waves
    finish them at very different times); a third without `y`, a third with
    one somewhere, a third with one as the last letter."""
    big = K > 33
    lay = Layout("split%d" % K, RX, (16 << 20) if big else (4 << 20), 512 if big else 128, seed=K)
    u = np.linspace(0.0, 1.0, K) if K > 1 else np.array([0.6])
    Ls = (4608 * (200 * 1024 / 4608) ** (u ** 3)).astype(np.int64)
    lay.rng.shuffle(Ls)
    b = 0
    for i, L in enumerate(Ls):
        d = D[i % 4]
        L = max(int(L), min_letters(d))
        end = lay.range_end(b)
        x = end - d
        ys = ((), (x + 1 + int(lay.rng.integers(0, L)),), (x + L,))[i % 3]
        lay.plant(b, d, L, ys)
        b = lay.next_record()
    lay.k = K
    lay.forest = K > COOP_MAX
    return lay.freeze()


ACCEPT_CASES = 7


def accepts(rx, zmix, K=33):
    """K plants in one scan; plant i's last accept lies, by i % 7: nowhere;
    before the range end only; inside the slack; inside R1's budget with
    letters going on; beyond R1's budget only; several `y`, the last one in the
    final partial 1 KiB round of R1b; the last letter.  zmix: every other walk
    is ended by `Z` (RX2's second accept index) instead of a blank."""
    lay = Layout("accepts" + ("Z" if zmix else ""), rx, 4 << 20, 128, seed=7 + zmix)
    rng = lay.rng
    b, seen = 0, [0] * ACCEPT_CASES
    for i in range(K):
        cat = i % ACCEPT_CASES
        nth = seen[cat]
        seen[cat] += 1
        d = D[(i + i // ACCEPT_CASES) % 4]
        if cat == 1 and d == 1:
            d = 17
        L = min_letters(d) + 2048 + int(rng.integers(0, 50000))
        end = lay.range_end(b)
        x, q0 = end - d, end + SLACK + CONV
        die = x + 1 + L
        if cat == 5 and (die - q0) % 1024 < 8:
            L, die = L + 8, die + 8
        edge = lambda lo, hi: lo if nth == 0 else hi - 1 if nth == 1 else int(rng.integers(lo, hi))
        if cat == 0:
            ys = ()
        elif cat == 1:
            ys = (edge(x + 1, end),)
        elif cat == 2:
            ys = (edge(end, end + SLACK),)
        elif cat == 3:
            ys = (edge(end + SLACK, q0),)
        elif cat == 4:
            ys = (edge(q0, die - 1),)
        elif cat == 5:
            fr = q0 + (die - q0) // 1024 * 1024
            ys = (x + 1 + d // 2, end + SLACK + 100, q0 + 17, fr + (die - fr) // 2)
        else:
            ys = (die - 1,)
        lay.plant(b, d, L, ys, kill=b"Z" if zmix and i % 2 else b" ")
        b = lay.next_record()
    lay.k = K
    return lay.freeze()


def wrong_guesses(K=24):
    """RX5 over walks of 5 to 40 KiB: an entry guessed from 4 bytes is wrong in
    four lanes of five, so each round of coop_continue advances by its
    wrong-guess path.  `y` after a multiple of 5 letters accepts, any other is
    a letter; by i % 3 the plant has only such letters, ends in an accepting
    one, or has an accepting one followed by others."""
    lay = Layout("guess5", RX5, 4 << 20, 128, seed=5)
    rng = lay.rng
    b = 0
    for i in range(K):
        d = D[i % 4]
        L = max(min_letters(d), int(rng.integers(5 << 10, 40 << 10)))
        x = lay.range_end(b) - d
        at = lambda t, good: x + 1 + (t // 5 * 5 if good else t // 5 * 5 + 1 + t % 4)   # letters before the y
        t = sorted(int(v) for v in rng.integers(5, L - 5, 4))
        if i % 3 == 0:
            ys = [at(v, False) for v in t]
        elif i % 3 == 1:
            ys = [at(t[0], False), at(t[1], True), at(t[2], False), at(L - 1, True)]
        else:
            ys = [at(t[0], True), at(t[1], False), at(t[2], True), at(t[3], False)]
        lay.plant(b, d, L, ys)
        b = lay.next_record()
    lay.k = K
    return lay.freeze()


def readable_end(halo):
    """Two ordinary plants, then one whose letters run to the end of the
    buffer.  halo: the scanned and readable range ends `tail` bytes before
    that (Scanner.scan with at_eof false); else it is the end of the input.
    (The last plant's match covers three records: the stitch takes a round
    for each, and gives up after 256 KiB / the record size of them.)"""
    n = (1 << 20) - 1000 if halo else (1 << 20) + 7
    lay = Layout("halo" if halo else "eof", RX, n, 32, seed=11, tail=2000 if halo else 0)
    lay.plant(1, 17, 9000, (lay.range_end(1) + 8000,))
    lay.plant(5, 255, 70000)
    b = lay.nrec - 4
    x = lay.range_end(b) - 100
    L = n + lay.tail - x - 1
    lay.plant(b, 100, L, (x + 1 + L // 2, n + lay.tail - 500 if halo else n - 5000))
    lay.k = 3
    return lay.freeze()


RUNS = (3, 40, 17, 58, 9, 25, 33, 5, 44, 12, 21, 30, 7, 37, 15, 28, 11, 19, 26, 2)   # open records of each run
RUN_OFFSETS = (0, 3, 255, 256, 257, 1000, 4000)


def chains():
    """Letter runs across many records.  Every record of a run but the first
    holds an `x` within its first 4000 bytes (and another 20 KiB further on),
    so each wave's open walk converges with its successor's in R1 (the walk V
    brought forward to W, or started beside it); the run then goes on without
    `x` for more than R1's budget, so the last open walk is R1b's, and R2
    carries its end back through the chain.  The only `y` of a run is its last
    letter; every fourth run has none."""
    lay = Layout("chains", RX, 16 << 20, 512, seed=13)
    rng = lay.rng
    b = 0
    lay.runs = []
    for i, m in enumerate(RUNS):
        d = D[i % 4]
        last = b + m - 1
        extra = min_letters(0) + int(rng.integers(0, 30000))      # letters behind the last open record's range
        x = lay.range_end(b) - d
        L = lay.range_end(last) + extra - x - 1
        p = lay.plant(b, d, L, () if i % 4 == 3 else (x + L,))
        for r in range(b + 1, last + 1):
            at = lay.range_start(r) + RUN_OFFSETS[(r + i) % len(RUN_OFFSETS)]
            lay.host[at] = ord("x")
            lay.host[at + 20000] = ord("x")
        lay.runs.append((b, last, p))
        b = lay.next_record()
    lay.k = len(RUNS)
    return lay.freeze()


def budget(mib=65):
    """One walk over 64 MiB + 1 MiB of letters: past kOpenCoopBudget R1b gives
    up (mib=63: it does not).  The walk has no `y`: a match across that many
    records would send the stitch to the forest FIND by itself (a round per
    record it covers).  Three short plants with matches follow it."""
    lay = Layout("budget%d" % mib if mib != 65 else "budget", RX, 80 << 20, 512, seed=17)
    lay.plant(3, 17, mib << 20)
    for i in range(3):
        b = lay.next_record()
        x = lay.range_end(b) - D[i + 1]
        lay.plant(b, D[i + 1], 6000 + 20000 * i, (x + 5500 + 20000 * i,))
    lay.k = 4
    lay.forest = (mib << 20) > COOP_BUDGET
    return lay.freeze()


SPLIT_K = (1, 16, 17, 33, 100, 256, 257)

CASES = dict([("split%d" % K, functools.partial(wave_split, K)) for K in SPLIT_K] + [
    ("accepts", functools.partial(accepts, RX, False)),
    ("acceptsZ", functools.partial(accepts, RX2, True)),
    ("guess5", wrong_guesses),
    ("eof", functools.partial(readable_end, False)),
    ("halo", functools.partial(readable_end, True)),
    ("chains", chains),
    ("budget63", functools.partial(budget, 63)),
    ("budget", budget),
])


@functools.lru_cache(maxsize=None)
def layout(name):
    """The named layout, built once (its buffer is read-only)."""
    return CASES[name]()
