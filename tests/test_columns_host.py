"""CPU: the models of the column semantics (tests/columns_model.py) against the
reference's rows (tests/golden/columns_cases.json: its recorded
Hello_*--csv-onkb.out and its CLI over columns_mix.bin with --tabs=1,2,4,8),
the stitched model against the direct one, and the argument checks
ugpu_columns makes before it touches a device.  The first two guard the
fixture and the model the GPU tests compare with."""
import ctypes
import json
import os

import numpy as np
import pytest

import columns_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(GOLDEN, "columns_cases.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def mix():
    return np.fromfile(os.path.join(GOLDEN, "columns_mix.bin"), np.uint8)


def _check_rows(data, tab, rows):
    """rows: [line, column, offset] as printed (1-based line and column)."""
    col, bol, line = M.direct(data, tab)
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    off = rows[:, 2]
    assert np.array_equal(np.asarray(line)[off], rows[:, 0])
    assert np.array_equal(np.asarray(col)[off], rows[:, 1] - 1)
    # bol-consistent: the line begins behind a newline (or the buffer), and no newline lies in [bol, offset)
    nl = np.concatenate([[0], np.cumsum(data == 10)])
    b = np.asarray(bol)[off]
    assert np.all(b <= off) and np.all((b == 0) | (data[np.maximum(b, 1) - 1] == 10))
    assert np.array_equal(nl[off], nl[b]) and np.array_equal(nl[b] + 1, rows[:, 0])


def test_direct_model_reproduces_recorded_outputs(cases):
    seen = 0
    for c in cases["recorded"]:
        for name in sorted({r[0] for r in c["rows"]}):
            data = np.fromfile(os.path.join(GOLDEN, "verify", name), np.uint8)
            rows = [r[1:] for r in c["rows"] if r[0] == name]
            _check_rows(data, c["tab"], rows)
            seen += len(rows)
    assert seen == 350


@pytest.mark.parametrize("tab", TABS)
def test_direct_model_reproduces_cli_rows(cases, mix, tab):
    rows = cases["mix"]["rows"][str(tab)]
    assert len(rows) == int(np.count_nonzero(mix == ord("x")))
    _check_rows(mix, tab, rows)
    at = bytes(bytearray(mix)).index(b"\t" * 4096) + 4096
    assert [r[1] for r in rows if r[2] == at] == [4096 * tab + 1]    # the x behind the line of 4096 tabs


def test_mix_holds_what_it_should(mix):
    assert mix.size <= 24 << 10
    nl = np.flatnonzero(mix == 10)
    lines = [bytes(bytearray(mix[a + 1:b])) for a, b in zip(nl[:-1], nl[1:])]
    assert any(len(ln) == 9000 and b"\t" not in ln for ln in lines)
    assert b"\t" * 4096 + b"x" in lines
    for byte in (9, 10, 13, 0xC3, 0xE2, 0xFF, 0x80):
        assert np.any(mix == byte), byte


@pytest.mark.parametrize("tab", TABS)
def test_numpy_model_equals_direct(mix, tab):
    want = M.direct(mix, tab)
    got = M.direct_np(mix, tab)
    for a, b in zip(got, want):
        assert a.tolist() == list(b)
    # a line that began before the data: the column carried in
    nl = np.flatnonzero(mix == 10)
    q = int(nl[np.flatnonzero(np.diff(nl) == 9001)[0]]) + 1 + 100   # 100 bytes into the long line
    k0 = want[0][q]
    assert k0 > 0
    col = M.direct_np(mix[q:], tab, k0)[0]
    assert col[:8901].tolist() == list(want[0][q:q + 8901])


@pytest.mark.parametrize("per", [16, 48, 4096, 8192])
@pytest.mark.parametrize("tab", TABS)
def test_stitched_model_equals_direct(mix, tab, per):
    want = M.direct(mix, tab)
    got = M.stitched(mix, tab, per)
    for a, b in zip(got, want):
        assert list(a) == list(b)


def test_stitched_model_small():
    for raw in (b"", b"\n", b"\t", b"a\tb\n\t\tc", b"\xe2\x82\xac\t\n\n\xff\x80\ra"):
        data = np.frombuffer(raw, np.uint8)
        for tab in TABS:
            for per in (1, 2, 3, 16):
                assert tuple(map(list, M.stitched(data, tab, per))) == tuple(map(list, M.direct(data, tab))), raw
    assert M.direct(np.frombuffer(b"a\tb\n\tc", np.uint8), 8) == ([0, 1, 8, 9, 0, 8, 9], [0, 0, 0, 0, 4, 4, 4],
                                                                [1, 1, 1, 1, 2, 2, 2])
    col, bol, line = M.expected(np.frombuffer(b"ab\n", np.uint8), [0, 3, 3, 4])
    assert col.tolist() == [0, 0, 0, M.FULL] and bol.tolist() == [0, 3, 3, M.FULL] and line.tolist() == [1, 2, 2, M.FULL]


# ---- argument checks made before any device call (no GPU here)

def _columns(tab, col, bol, line):
    from ugrep_amd import _lib
    V = ctypes.c_void_p
    fake = 1 << 20   # a 16-byte aligned address that is never read
    return _lib, _lib.lib.ugpu_columns(V(fake), 64, V(fake), 1, tab, V(col), V(bol), V(line), None)


@pytest.mark.parametrize("tab", [0, 3, 5, 6, 7, 9, 16])
def test_bad_tab_is_inval(tab):
    _lib, rc = _columns(tab, 1 << 20, 1 << 20, 1 << 20)
    assert rc == _lib.UGPU_INVAL
    assert b"tab" in _lib.lib.ugpu_last_error()


def test_no_output_is_inval():
    _lib, rc = _columns(8, None, None, None)
    assert rc == _lib.UGPU_INVAL


def test_header_declares_columns():
    from ugrep_amd import _lib
    assert "ugpu_columns" in _lib.declared_symbols()
    assert _lib.lib.ugpu_abi_version() == 3
