"""CPU: the models of the input conversions (tests/transcode_model.py) against
the reference CLI's recorded outputs (tests/golden/transcode_cases.json), the
stitched model against the direct one, ugpu_detect_bom and
ugpu_transcode_bound against the table, and the argument checks
ugpu_transcode makes before it touches a device.  The first two guard the
fixture and the model the GPU tests compare with."""
import ctypes

import numpy as np
import pytest

import transcode_model as M
from transcode_model import ENCS, load_cases, printed, random_input, random_page


@pytest.fixture(scope="module")
def golden():
    return load_cases()


def test_direct_model_reproduces_recorded_outputs(golden):
    cases, _ = golden
    assert len(cases) == 41
    for name, data, enc, skip, page, out in cases:
        assert printed(M.direct(data[skip:], enc, page)) == out, name
    seen = {enc for _, _, enc, _, _, _ in cases}
    assert seen == set(ENCS)


def test_recorded_cases_hold_what_they_should(golden):
    cases, g = golden
    by = {c[0]: c for c in cases}
    for order in ("le", "be"):
        body = M.direct(by["utf16%s_body" % order][1][2:], M.NAMES["utf16" + order])
        assert body.count(M.NONCHAR) >= 20 and "\U0001F600".encode() in body and b"\xf4\x8f\xbf\xbf" in body
        assert M.direct(by["utf16%s_tail2_low" % order][1][2:], M.NAMES["utf16" + order]).endswith(b"\xf0\x90\x90\x85")
        for t in ("tail0", "tail1", "tail2_bmp", "tail3_bmp"):
            assert M.direct(by["utf16%s_%s" % (order, t)][1][2:], M.NAMES["utf16" + order]) == b"Ax\n" + M.NONCHAR, t
        b32 = M.direct(by["utf32%s_body" % order][1][4:], M.NAMES["utf32" + order])
        assert b32.endswith(b"x" + M.NONCHAR + b"\nxA\nx\xff\n") and b"x\xed\xa0\x80\n" in b32
    assert len(by["latin1_all"][1]) == 258
    for key in ("cp1252", "koi8r"):
        page = g["pages"][key]
        assert len(page) == 256 and page[:0x80] == list(range(0x80)) and page.count(10) == 1
    assert g["pages"]["cp1252"][0x80] == 0x20AC and g["pages"]["koi8r"][0xC1] == 0x430


@pytest.mark.parametrize("enc", ENCS)
def test_stitched_model_equals_direct(enc):
    rng = np.random.default_rng(100 + enc)
    w = 2 if enc in (M.UTF16BE, M.UTF16LE) else 4 if enc in (M.UTF32BE, M.UTF32LE) else 1
    page = random_page(rng) if enc == M.PAGE else None
    for n in (0, 1, 2, 3, 5, 64, 257, 1000, 1003):
        data = random_input(rng, enc, n)
        want = M.direct(data, enc, page)
        for per in (1, 3, 5, 7, 33):
            assert M.stitched(data, enc, page, per * w) == want, (n, per)


@pytest.mark.parametrize("order", [M.UTF16BE, M.UTF16LE])
def test_stitched_model_through_runs(order):
    """Ranges that are H units throughout: the XOR carry."""
    fmt = ">u2" if order == M.UTF16BE else "<u2"
    for m in (1, 2, 7, 8, 30, 31):
        for tail in ([], [0xDC00], [0xDC00, 0x41], [0x41, 0x42], [0xDC00, 0xDC00]):
            data = np.asarray([0xD800] * m + tail).astype(fmt).tobytes()
            want = M.direct(data, order)
            for per in (2, 6, 10, 16):
                assert M.stitched(data, order, None, per) == want, (m, tail, per)
    assert M.direct(np.asarray([0xD800, 0xD800, 0xDC00, 0x41]).astype(fmt).tobytes(), order) == M.NONCHAR * 2 + b"A"
    assert M.direct(np.asarray([0xD800, 0xD800, 0xD800, 0xDC00, 0x41]).astype(fmt).tobytes(), order) == \
        M.NONCHAR + b"\xf0\x90\x80\x80A"


# ---- the host calls

def _lib():
    from ugrep_amd import _lib
    return _lib


def test_detect_bom(golden):
    L = _lib()
    _, g = golden
    names = dict(M.NAMES, plain=M.PLAIN, utf8=M.UTF8)
    assert {r["enc"] for r in g["bom"]} == {"plain", "utf8", "utf16be", "utf16le", "utf32be", "utf32le"}
    for r in g["bom"]:
        head = bytes.fromhex(r["head"])
        enc, skip = ctypes.c_uint32(9), ctypes.c_uint32(9)
        buf = (ctypes.c_uint8 * 4)(*head[:4])
        assert L.lib.ugpu_detect_bom(buf, len(head), ctypes.byref(enc), ctypes.byref(skip)) == L.UGPU_OK
        assert (enc.value, skip.value) == (names[r["enc"]], r["skip"]) == M.detect_bom(head[:4], len(head)), r["head"]
        if "out" in r:   # the CLI over the head: the conversion the row announces
            want = head[skip.value:] if enc.value == M.UTF8 else M.direct(head[skip.value:], enc.value)
            assert printed(want) == bytes.fromhex(r["out"]), r["head"]
    # the length, not the bytes behind it, decides FF FE
    buf = (ctypes.c_uint8 * 4)(0xFF, 0xFE, 0x41, 0x00)
    enc, skip = ctypes.c_uint32(), ctypes.c_uint32()
    for n, want in ((2, (M.PLAIN, 0)), (3, (M.PLAIN, 0)), (4, (M.UTF16LE, 2)), (1 << 33, (M.UTF16LE, 2))):
        assert L.lib.ugpu_detect_bom(buf, n, ctypes.byref(enc), ctypes.byref(skip)) == L.UGPU_OK
        assert (enc.value, skip.value) == want
    assert L.lib.ugpu_detect_bom(None, 0, ctypes.byref(enc), ctypes.byref(skip)) == L.UGPU_OK
    assert (enc.value, skip.value) == (M.PLAIN, 0)


def test_transcode_bound():
    L = _lib()
    b = ctypes.c_uint64()
    for enc in ENCS:
        for n in (0, 1, 2, 3, 4, 7, 4096, (1 << 32) + 5):
            assert L.lib.ugpu_transcode_bound(enc, n, ctypes.byref(b)) == L.UGPU_OK
            assert b.value == M.bound(enc, n), (enc, n)
    for enc in (M.PLAIN, M.UTF8, 9, 1000):
        assert L.lib.ugpu_transcode_bound(enc, 8, ctypes.byref(b)) == L.UGPU_INVAL
    rng = np.random.default_rng(7)
    for enc in ENCS:     # the bound holds, and the worst inputs reach it
        page = [0x800 + i for i in range(256)] if enc == M.PAGE else None
        assert len(M.direct(random_input(rng, enc, 999), enc, page)) <= M.bound(enc, 999)
    assert len(M.direct(b"\xdc\x00" * 8, M.UTF16BE)) == M.bound(M.UTF16BE, 16)
    assert len(M.direct(b"\x7f\xff\xff\xff" * 4, M.UTF32BE)) == M.bound(M.UTF32BE, 16)
    assert len(M.direct(b"\xe9" * 16, M.LATIN1)) == M.bound(M.LATIN1, 16)
    assert len(M.direct(b"\xe9" * 16, M.PAGE, [0x20AC] * 256)) == M.bound(M.PAGE, 16)


def _transcode(enc, page=None, length=64, start=0, dst=1 << 20):
    L = _lib()
    V = ctypes.c_void_p
    fake = 1 << 20   # a 16-byte aligned address that is never read
    out = ctypes.c_uint64(77)
    pg = None if page is None else (ctypes.c_uint16 * 256)(*page)
    return L, L.lib.ugpu_transcode(V(fake), length, start, enc, pg, V(dst), 1 << 20, ctypes.byref(out), None), out.value


@pytest.mark.parametrize("enc", [M.PLAIN, M.UTF8, 9, 255, 1 << 31])
def test_nothing_to_convert_is_inval(enc):
    L, rc, _ = _transcode(enc)
    assert rc == L.UGPU_INVAL
    assert b"encoding" in L.lib.ugpu_last_error()


def test_page_argument_is_checked():
    L, rc, _ = _transcode(M.PAGE)
    assert rc == L.UGPU_INVAL and b"page" in L.lib.ugpu_last_error()
    for enc in (M.UTF16LE, M.UTF32BE, M.LATIN1, M.NULL_DATA):
        L, rc, _ = _transcode(enc, page=list(range(256)))
        assert rc == L.UGPU_INVAL and b"page" in L.lib.ugpu_last_error()


def test_start_behind_the_input_is_inval():
    L, rc, _ = _transcode(M.LATIN1, length=64, start=65)
    assert rc == L.UGPU_INVAL and b"start" in L.lib.ugpu_last_error()


def test_nothing_to_read_gives_zero():
    for enc in ENCS:
        L, rc, out = _transcode(enc, page=list(range(256)) if enc == M.PAGE else None, length=64, start=64)
        assert (rc, out) == (L.UGPU_OK, 0)


def test_header_declares_transcode():
    L = _lib()
    assert {"ugpu_detect_bom", "ugpu_transcode_bound", "ugpu_transcode"} <= set(L.declared_symbols())
    assert L.lib.ugpu_abi_version() == 3
