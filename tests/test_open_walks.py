"""GPU: open walks that fix_kernel's R1 cannot resolve (scan_kernels.hip
resolve_open, R1b: coop_continue, one wave per walk).

The layouts (tests/open_walks.py; tests/test_open_walks_host.py proves how
many unresolved walks each holds) plant walks that are alive at their wave's
range end and stay alive, alone, past R1's budget.  Each scan is compared with
the oracle: totals in COUNT mode, every record of find_all (the WRITE pass
takes the match ends from the OpenRec), one layout through find_records and
one through Stream.feed.  Whether R1b did the work shows in UGPU_TOT_FOREST of
Scanner.totals(): a walk no wave took, or one past the budgets, sends the scan
to the forest FIND, which is exact too.

Hazard -> test:
  the split of the walks over the block's 16 waves  test_wave_split (K = 17 .. 256: more walks
                                                    than waves, finished at very different times)
  coop_continue's accept path, the last accept R1   test_where_the_last_accept_lies, test_accept_index
  hands over, death and accept in one round
  its wrong-guess path                              test_wrong_guesses
  the readable end, with EOF and without            test_readable_end, test_readable_end_before_eof
  kOpenCoopMax (256 against 257 walks)              test_wave_split[256], [257]
  kOpenCoopBudget (63 MiB against 65 MiB)           test_walk_under_the_budget, test_walk_budget
  R2's carry through a chain whose last link is     test_chains_end_in_r1b
  R1b's
"""
import contextlib
import os
import time

import pytest

import open_walks as OW

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FOREST = 8   # UGPU_TOT_FOREST


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def _grid(n):
    """UGPU_MAX_GRID is read when a scanner is created: the pattern (and with
    it the pool find_all, find_records and Stream take theirs from) is made
    inside."""
    os.environ["UGPU_MAX_GRID"] = str(n)
    try:
        yield
    finally:
        os.environ.pop("UGPU_MAX_GRID", None)


_WANT = {}


def _want(U, lay):
    """The oracle's (count, digest, dcap, triples) of a layout, computed once."""
    from oracle_lib import OracleDfa
    if lay.name not in _WANT:
        _WANT[lay.name] = OracleDfa(U.compile_regex(lay.rx)).find(lay.host[:lay.n], want_list=True)
    return _WANT[lay.name]


def _pattern(U, lay):
    pat = U.Pattern(U.compile_regex(lay.rx))
    assert pat.info()["kernel"] == 0, "expected the prefiltered kernel for %r" % lay.rx
    return pat


def _device(lay):
    dev = torch.zeros(lay.host.size + 64, dtype=torch.uint8, device="cuda")
    dev[:lay.host.size].copy_(torch.from_numpy(lay.host))
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    return dev


def _check(U, name):
    """COUNT totals and FOREST flag of a Scanner scan, the records of find_all
    and its COUNT mode, against the oracle."""
    lay = OW.layout(name)
    want = _want(U, lay)
    with _grid(lay.grid):
        pat = _pattern(U, lay)
        dev = _device(lay)
        sc = U.Scanner(pat)
        t0 = time.perf_counter()
        sc.scan(dev.data_ptr(), 0, lay.n, lay.n, True, 0, _stream())
        t = sc.totals()
        dt = time.perf_counter() - t0
        got = U.find_all(pat, dev[:lay.n], offsets=True)
        cnt = U.find_all(pat, dev[:lay.n], offsets=False)
        sc.close()
    print("%s: %d walks for R1b, %d matches (%d expected), flags %#x, scan + totals %.1f ms"
          % (name, lay.k, t.count, want[0], t.flags, dt * 1e3))
    assert (t.count, t.digest, t.dcap) == tuple(want[:3]), name
    assert (cnt.count, cnt.digest, cnt.dcap) == tuple(want[:3]), name
    assert (got.count, got.digest, got.dcap) == tuple(want[:3]), name
    assert got.triples() == want[3], name
    assert bool(t.flags & FOREST) == lay.forest, "%s: %d unresolved walks, flags %#x" % (name, lay.k, t.flags)
    return dt


@pytest.mark.parametrize("K", OW.SPLIT_K)
def test_wave_split(U, K):
    """K walks for R1b in one scan, 4.5 KiB to 200 KiB long in shuffled order:
    each is walked by one of the block's 16 waves (FOREST clear, up to
    kOpenCoopMax = 256 walks); with 257 none is and the forest FIND answers."""
    _check(U, "split%d" % K)


def test_where_the_last_accept_lies(U):
    """33 walks whose last accept lies nowhere, before the range end, in the
    slack, in R1's budget (R1 hands lastw / lew to R1b, which finds nothing
    later), beyond it, in the final partial round of R1b, and on the last
    letter (accept and death in one lane of one round)."""
    _check(U, "accepts")


def test_accept_index(U):
    """The same with two accept indices, every other walk ended by the second
    one's `Z`: lew / le_e reach dcap and the records' cap field."""
    _check(U, "acceptsZ")
    assert {c for _, _, c in _want(U, OW.layout("acceptsZ"))[3]} == {1, 2}


def test_wrong_guesses(U):
    """`x([a-z]{5})*y` (kernel 0): the entry state depends on the number of
    letters mod 5, which the 4 bytes before a lane's 16 do not tell, so
    coop_continue advances to the first wrong lane round after round."""
    _check(U, "guess5")


def test_readable_end(U):
    """A walk R1b follows to the end of the input (EOF): it ends there, with its last accept."""
    _check(U, "eof")


def test_readable_end_before_eof(U):
    """The same walk with the readable end before EOF: the scan cannot know
    the match's end and says UGPU_HALO; with the bytes behind the range
    readable (and EOF after them) R1b walks on past the range's end."""
    from oracle_lib import range_totals
    from ugrep_amd._lib import UGPU_HALO, UgpuError
    lay = OW.layout("halo")
    with _grid(lay.grid):
        pat = _pattern(U, lay)
        dev = _device(lay)
        sc = U.Scanner(pat)
        sc.scan(dev.data_ptr(), 0, lay.n, lay.n, False, 0, _stream())
        with pytest.raises(UgpuError) as e:
            sc.totals()
        assert e.value.code == UGPU_HALO
        sc.scan(dev.data_ptr(), 0, lay.n, lay.n + lay.tail, True, 0, _stream())
        t = sc.totals()
        sc.close()
    want = range_totals(U.compile_regex(lay.rx), lay.host, 0, lay.n)
    assert want[3] > lay.n
    assert (t.count, t.digest, t.dcap, t.exit) == want
    assert not t.flags & FOREST


def test_chains_end_in_r1b(U):
    """20 letter runs across 2 to 58 records each: every open walk of a run
    converges with the next one's in R1, the last is R1b's, and R2 carries its
    end (or that there is none) back through the chain, across its groups of
    64 records."""
    _check(U, "chains")


def test_walk_under_the_budget(U):
    """One walk over 63 MiB of letters (80 MiB buffer): one wave of fix_kernel
    walks it all, about 65 000 dependent rounds of 1 KiB (0.32 s on an MI355X)."""
    _check(U, "budget63")


def test_walk_budget(U):
    """One walk over 64 MiB + 1 MiB of letters: past kOpenCoopBudget R1b gives
    up and the forest FIND answers, exactly.  The forest FIND walks such a run
    at about 0.36 s a MiB: 23.5 s for the COUNT scan and as long again for the
    records, so this test takes the totals and the records of one Scanner scan
    (the WRITE pass find_all runs) instead of _check's three scans, and still
    takes 59 s: the slowest test of the suite, kept because nothing else shows
    that a walk past the budget is given up and not cut short."""
    lay = OW.layout("budget")
    want = _want(U, lay)
    with _grid(lay.grid):
        pat = _pattern(U, lay)
        dev = _device(lay)
        sc = U.Scanner(pat)
        t0 = time.perf_counter()
        sc.scan(dev.data_ptr(), 0, lay.n, lay.n, True, 0, _stream())
        t = sc.totals()
        t1 = time.perf_counter()
        n = int(t.count)
        s = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ln = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        cp = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        sc.offsets(s.data_ptr(), ln.data_ptr(), cp.data_ptr(), n + 1, _stream())
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        sc.close()
    print("budget: flags %#x, scan + totals %.2f s, records %.2f s" % (t.flags, t1 - t0, t2 - t1))
    assert (t.count, t.digest, t.dcap) == tuple(want[:3])
    assert [list(r) for r in zip(s[:n].tolist(), ln[:n].tolist(), cp[:n].tolist())] == want[3]
    assert t.flags & FOREST


def test_find_records(U):
    """The records path (chunked input, scans from the true chain entry) over the two-index layout."""
    lay = OW.layout("acceptsZ")
    want = _want(U, lay)
    os.environ["UGPU_REC_CHUNK"] = str(1 << 20)
    try:
        with _grid(lay.grid):
            pat = _pattern(U, lay)
            r = U.Records(pat, lay.host)
            assert r.totals() == tuple(want[:3])
            assert r.triples() == want[3]
            r.close()
    finally:
        os.environ.pop("UGPU_REC_CHUNK", None)


def test_stream_feed(U):
    """Stream.feed in 512 KiB chunks over 33 walks of up to 200 KiB: walks open at a chunk's end too."""
    lay = OW.layout("split33")
    want = _want(U, lay)
    step = 512 << 10
    with _grid(lay.grid):
        pat = _pattern(U, lay)
        st = U.Stream(pat)
        recs = []
        for k in range(0, lay.n, step):
            recs += st.feed(lay.host[k:k + step], final=k + step >= lay.n).triples()
        st.close()
    assert recs == want[3]
