"""GPU: ugpu_columns (column, line begin and line of byte positions; ugrep -k,
--tabs) against the reference's rows (tests/golden/columns_cases.json) and the
models of tests/columns_model.py, which tests/test_columns_host.py ties to
those rows.  Every comparison is exact.  At these sizes every 4 KiB tile is its
own wave range, so a buffer of 64 KiB is 16 ranges stitched on the host."""
import json
import os

import numpy as np
import pytest

import columns_model as M
import highpos as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABS = (1, 2, 4, 8)
U64 = np.uint64
FULL = U64(M.FULL)


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "columns_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def mix():
    return np.fromfile(os.path.join(GOLDEN, "columns_mix.bin"), np.uint8)


def _file(name):
    return np.fromfile(os.path.join(GOLDEN, "verify", name), np.uint8)


def _dev(data, slack=b""):
    """The data in a 16-byte aligned device buffer with a readable last granule
    (`slack`: the bytes behind len, zero when not given)."""
    data = np.asarray(data, np.uint8)
    buf = torch.zeros(data.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if data.size:
        buf[:data.size] = torch.from_numpy(data.copy())
    if slack:
        buf[data.size:data.size + len(slack)] = torch.from_numpy(np.frombuffer(slack, np.uint8).copy())
    return buf


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, U64)).view(np.int64).copy()).to("cuda")


def _columns(U, ptr, n, pos, tab, want=(True, True, True)):
    """(col, bol, line) uint64 arrays of ugpu_columns; None where not asked for.
    The output arrays are preset to a pattern no result can equal."""
    pos = np.asarray(pos, U64)
    d_pos = _dev64(pos) if pos.size else None
    outs = [torch.full((max(pos.size, 1),), -2, dtype=torch.int64, device="cuda") if w else None for w in want]
    torch.cuda.synchronize()
    U.columns(ptr, n, d_pos.data_ptr() if pos.size else 0, pos.size, tab,
              *[o.data_ptr() if o is not None else 0 for o in outs])
    return tuple(None if o is None else o[:pos.size].cpu().numpy().view(U64) for o in outs)


def _check(U, data, pos, tab, slack=b""):
    data = np.asarray(data, np.uint8)
    buf = _dev(data, slack)
    got = _columns(U, buf.data_ptr(), data.size, pos, tab)
    want = M.expected(data, pos, tab)
    for name, g, w in zip(("col", "bol", "line"), got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (name, tab, int(np.asarray(pos)[bad[0]]), int(g[bad[0]]), int(w[bad[0]]), bad.size)
    return got


# ---- the reference's rows

def test_recorded_rows(U, golden):
    seen = 0
    for c in golden["recorded"]:
        for name in sorted({r[0] for r in c["rows"]}):
            data = _file(name)
            rows = np.asarray([r[1:] for r in c["rows"] if r[0] == name], np.int64)
            buf = _dev(data)
            col, bol, line = _columns(U, buf.data_ptr(), data.size, rows[:, 2], c["tab"])
            assert np.array_equal(col + U64(1), rows[:, 1].astype(U64)), (c["pattern"], name)
            assert np.array_equal(line, rows[:, 0].astype(U64)), (c["pattern"], name)
            want_bol = np.asarray(M.direct(data, c["tab"])[1], np.int64)[rows[:, 2]]
            assert np.array_equal(rows[:, 2].astype(U64) - bol, (rows[:, 2] - want_bol).astype(U64)), (c["pattern"], name)
            seen += len(rows)
    assert seen == 350


@pytest.mark.parametrize("tab", TABS)
def test_cli_rows(U, golden, mix, tab):
    rows = np.asarray(golden["mix"]["rows"][str(tab)], np.int64)
    buf = _dev(mix)
    col, bol, line = _columns(U, buf.data_ptr(), mix.size, rows[:, 2], tab)
    assert np.array_equal(col + U64(1), rows[:, 1].astype(U64))
    assert np.array_equal(line, rows[:, 0].astype(U64))
    want_bol = np.asarray(M.direct(mix, tab)[1], np.int64)[rows[:, 2]]
    assert np.array_equal(rows[:, 2].astype(U64) - bol, (rows[:, 2] - want_bol).astype(U64))


def test_find_positions_recorded_rows(U, golden, patterns):
    seen = 0
    for c in golden["recorded"]:
        if c["patterns_key"] not in ("hello", "hello_wnhS"):
            continue
        pat = U.Pattern(patterns[c["patterns_key"]]["opc"])
        for name in sorted(os.listdir(os.path.join(GOLDEN, "verify"))):
            if not name.startswith(("Hello.", "empty")):
                continue   # (the recorded run covered Hello.* empty.txt emptyline.txt)
            r = U.find_positions(pat, _file(name).tobytes(), tab=c["tab"])
            got = [list(x) for x in zip(r.line.tolist(), (r.column + U64(1)).tolist(), r.start.tolist())]
            assert got == [x[1:] for x in c["rows"] if x[0] == name], (c["pattern"], name)
            assert r.length.size == r.cap.size == len(got)
            seen += len(got)
    assert seen == 10 + 217


# ---- every position, and the structures

@pytest.mark.parametrize("tab", TABS)
def test_every_position(U, mix, tab):
    n = (64 << 10) + 5
    data = np.tile(mix, n // mix.size + 1)[:n]
    slack = b"\t\n\t\n\t\n\t\n\t\n\t"      # the 11 bytes of the last granule behind len: ignored
    assert (n + len(slack)) % 16 == 0
    _check(U, data, np.arange(n + 1), tab, slack)


@pytest.mark.parametrize("what", ["tab", "nl", "utf3"])
@pytest.mark.parametrize("side", [0, 1])
def test_boundaries(U, what, side):
    """A tab, a newline and a three-byte character at the granule, quarter,
    tile and range boundaries 16, 1024, 4096, 8192: the byte at B - 1 (side 0)
    or at B (side 1); the character straddles B with one or two bytes before it."""
    data = np.frombuffer((b"ab\xc3\xa9d " * 2000)[:9000], np.uint8).copy()
    data[100] = 10
    for B in (16, 1024, 4096, 8192):
        if what == "utf3":
            data[B - 1 - side:B + 2 - side] = np.frombuffer("€".encode(), np.uint8)
        else:
            data[B - 1 + side] = 9 if what == "tab" else 10
        data[B - 5] = 9         # (a tab shortly before, so that the column is not the byte count)
    for tab in TABS:
        _check(U, data, np.arange(data.size + 1), tab)


@pytest.mark.parametrize("tab", TABS)
def test_one_line_across_ranges(U, tab):
    data = np.full(40 << 10, ord("a"), np.uint8)
    data[999::1000] = 9
    col, bol, line = _check(U, data, np.arange(data.size + 1), tab)
    assert np.all(bol == 0) and np.all(line == 1) and col[-1] > 4096 * 9


def test_two_tiles_of_tabs(U):
    data = np.concatenate([np.full(4095, ord("x"), np.uint8), [10], np.full(8192, 9, np.uint8), [ord("x")] * 3]).astype(np.uint8)
    col, bol, line = _check(U, data, np.arange(data.size + 1), 8)
    assert col[4096] == 0 and col[8192] == 32768 and col[12288] == 65536 and col[12290] == 65538
    assert bol[12290] == 4096 and line[12290] == 2


@pytest.mark.parametrize("byte", [0x80, 10])
def test_runs(U, byte):
    data = np.concatenate([np.frombuffer(b"a\tb", np.uint8), np.full(20 << 10, byte, np.uint8),
                           np.frombuffer(b"c\td", np.uint8)])
    for tab in (1, 8):
        col, bol, line = _check(U, data, np.arange(data.size + 1), tab)
    if byte == 0x80:
        assert col[3] == col[3 + (20 << 10)] == 9 and line[-1] == 1
    else:
        assert line[-1] == 1 + (20 << 10) and bol[-1] == 3 + (20 << 10)


# ---- edges

def test_no_positions(U):
    buf = _dev(np.frombuffer(b"abc\n", np.uint8))
    out = torch.full((4,), -2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    U.columns(buf.data_ptr(), 4, 0, 0, 8, out.data_ptr(), out.data_ptr(), out.data_ptr())
    assert out.cpu().tolist() == [-2] * 4


def test_empty_buffer(U):
    buf = _dev(np.zeros(0, np.uint8), b"\t\n")
    col, bol, line = _columns(U, buf.data_ptr(), 0, [0], 8)
    assert (col.tolist(), bol.tolist(), line.tolist()) == ([0], [0], [1])
    col, bol, line = _columns(U, buf.data_ptr(), 0, [0, 0, 1], 8)
    assert (col.tolist(), bol.tolist(), line.tolist()) == ([0, 0, M.FULL], [0, 0, M.FULL], [1, 1, M.FULL])


def test_repeats_and_past_the_end(U, mix):
    n = mix.size
    pos = np.sort(np.concatenate([np.repeat(np.arange(0, n, 97), 3), [0, 0, n - 1, n, n, n, n + 1, n + 1, 1 << 40]]))
    got = _check(U, mix, pos, 4)
    for a in got:
        assert a[-3:].tolist() == [M.FULL] * 3 and a[-4] != FULL
    pos = np.repeat(U64(4097), 200)     # more than a step of 64 at one position
    _check(U, mix, pos, 8)


@pytest.mark.parametrize("skip", [0, 1, 2])
def test_one_output_null(U, mix, skip):
    buf = _dev(mix)
    pos = np.arange(0, mix.size + 1, 13)
    want = [k != skip for k in range(3)]
    got = _columns(U, buf.data_ptr(), mix.size, pos, 8, want)
    exp = M.expected(mix, pos, 8)
    for k in range(3):
        assert (got[k] is None) if k == skip else np.array_equal(got[k], exp[k])


def test_sparse_list(U, mix):
    data = np.tile(mix, 4)[:64 << 10]
    _check(U, data, [5000, 61234], 8)
    _check(U, data, [64 << 10], 2)
    _check(U, data, [0], 2)


def test_line_equals_ugpu_lines(U, mix):
    data = np.tile(mix, 4)[:(64 << 10) + 5]
    pos = np.flatnonzero(data == ord("x"))
    buf = _dev(data)
    _, _, line = _columns(U, buf.data_ptr(), data.size, pos, 8)
    d_pos = _dev64(pos)
    d_line = torch.zeros(pos.size, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    U.lines(buf.data_ptr(), data.size, d_pos.data_ptr(), pos.size, d_line.data_ptr())
    assert np.array_equal(line, d_line.cpu().numpy().view(U64))


# ---- offsets past 2^31 and 2^32

def test_high_offsets(U):
    """The 2^32 + 1 MiB layout of tests/highpos.py: filler lines of 1 MiB, and
    two 2 MiB windows of text around the seams 2^31 and 2^32, here with tabs and
    a split three-byte character at the seam.  Expected values are the model's
    over the window and the filler line before it, moved by the offset and the
    lines before.  Positions and line begins pass 2^32; the line numbers of this
    layout stay small, and a line of 4 GiB or more, with a column past 2^32, is
    not tested."""
    L = H.full_layout()
    win = H.variant(L, H.base_window(L), "utf3")
    S = L.half
    win[[S - 40, S - 12, S + 20]] = 9
    nlw = np.flatnonzero(win == 10)
    win[int(nlw[nlw < S - 100][-1]) + 7] = 9       # a tab early in the line that crosses the seam
    buf = torch.empty(L.N + 16, dtype=torch.uint8, device="cuda")
    buf.fill_(H.F)
    buf[L.P - 1:L.N:L.P] = 10
    buf[L.N:] = 9
    t = torch.from_numpy(win).to("cuda")
    for w in range(len(L.seams)):
        buf[L.wbase(w):L.wend(w)].copy_(t)
    local = np.concatenate([np.full(L.P - 1, H.F, np.uint8), [10], win]).astype(np.uint8)
    rng = np.random.default_rng(5)
    rel = np.unique(np.concatenate([[0, 1, L.P - 1, L.P, L.P + 1], np.arange(L.P + S - 64, L.P + S + 65),
                                    rng.integers(0, local.size, 3000), [local.size - 1, local.size]]))
    pos, want = [], [[], [], []]
    for tab in (8,):
        mcol, mbol, mline = (a[rel] for a in M.direct_np(local, tab))
        for w in range(len(L.seams)):
            off = L.wbase(w) - L.P
            pos.append(rel.astype(U64) + U64(off))
            want[0].append(mcol.astype(U64))
            want[1].append(mbol.astype(U64) + U64(off))
            want[2].append(mline.astype(U64) + U64(L.newlines_before(w, win) - 1))
    pos = np.concatenate(pos + [np.asarray([L.N + 1], U64)])
    want = [np.concatenate(x + [np.asarray([FULL])]) for x in want]
    assert np.all(np.diff(pos.astype(np.int64)) >= 0)
    for tab in (8, 2):
        if tab == 2:
            want[0] = np.concatenate([M.direct_np(local, 2)[0][rel].astype(U64)] * 2 + [np.asarray([FULL])])
        got = _columns(U, buf.data_ptr(), L.N, pos, tab)
        for name, g, x in zip(("col", "bol", "line"), got, want):
            bad = np.flatnonzero(g != x)
            assert bad.size == 0, (name, tab, int(pos[bad[0]]), int(g[bad[0]]), int(x[bad[0]]), bad.size)
    assert np.any(got[1][:-1] > U64(1 << 32)) and np.any((got[1] > U64(1 << 31)) & (got[1] < U64(1 << 32)))
    assert got[2][-2] == U64(L.newlines_before(1, win) + np.count_nonzero(win == 10) + 1) and got[0][-2] == 0
    del buf
    torch.cuda.empty_cache()
