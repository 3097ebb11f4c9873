"""GPU: ugpu_transcode (UTF-16/32, Latin-1, code pages and null data into the
bytes the scans take) against the reference CLI's recorded outputs
(tests/golden/transcode_cases.json) and the models of tests/transcode_model.py,
which tests/test_transcode_host.py ties to those outputs.  Every comparison is
exact.  Below 16 MiB every 4 KiB tile is its own wave range, so an input of
64 KiB is 16 ranges stitched on the host."""
import numpy as np
import pytest

import transcode_model as M
from transcode_model import ENCS, load_cases, printed, random_input, random_page

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
U16 = (M.UTF16BE, M.UTF16LE)
U32 = (M.UTF32BE, M.UTF32LE)


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def golden():
    return load_cases()


def _dev(data, start=0):
    """`start` bytes of a pattern, then the data, in a 16-byte aligned device
    buffer whose last granule is readable; the bytes behind the data are high
    surrogates in both byte orders, which the call must ignore."""
    data = np.frombuffer(bytes(data), np.uint8)
    n = start + data.size
    buf = torch.full((n + 16,), 0xD8, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if data.size:
        buf[start:n] = torch.from_numpy(data.copy())
    return buf, n


def _convert(U, buf, n, enc, start=0, page=None, slack=64):
    """(output bytes, output length): the size query, then the conversion into
    a destination preset to SENTINEL, which must be untouched from out_len on."""
    torch.cuda.synchronize()
    m = U.transcode(buf.data_ptr(), n, enc, start, page)
    dst = torch.full((m + slack,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    assert U.transcode(buf.data_ptr(), n, enc, start, page, dst.data_ptr(), m) == m
    out = dst.cpu().numpy()
    assert np.all(out[m:] == SENTINEL), "bytes written behind out_len"
    return out[:m].tobytes(), m


def _check(U, data, enc, want, starts=(0,), page=None):
    for s in starts:
        buf, n = _dev(data, s)
        got, m = _convert(U, buf, n, enc, s, page)
        if got != want:
            a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
            k = min(a.size, b.size)
            bad = np.flatnonzero(a[:k] != b[:k])
            at = int(bad[0]) if bad.size else k
            raise AssertionError((enc, s, len(data), "lengths", a.size, b.size, "first difference at", at,
                                  got[max(at - 8, 0):at + 8].hex(), want[max(at - 8, 0):at + 8].hex()))


def _units16(enc, units):
    return np.asarray(units).astype(">u2" if enc == M.UTF16BE else "<u2").tobytes()


# ---- the reference's outputs

def test_recorded_cases(U, golden):
    """Every recorded case, the converted bytes placed at several offsets of
    the buffer (0 to 3: every byte shift of the loads; 16 and 18: past a granule)."""
    cases, _ = golden
    for name, data, enc, skip, page, out in cases:
        for s in (skip, 0, 1, 2, 3, 7, 16, 18):
            buf, n = _dev(data[skip:], s)
            got, _ = _convert(U, buf, n, enc, s, page)
            assert printed(got) == out, (name, s)


def test_in_place_with_bom_skip(U, golden):
    """The files as they are, start = the BOM's length."""
    cases, _ = golden
    for name, data, enc, skip, page, out in cases:
        buf, n = _dev(data, 0)
        assert n == len(data)
        got, _ = _convert(U, buf, n, enc, skip, page)
        assert printed(got) == out, name


# ---- size query, capacity, edges

@pytest.mark.parametrize("enc", ENCS)
def test_size_query_and_capacity(U, enc):
    rng = np.random.default_rng(enc)
    page = random_page(rng) if enc == M.PAGE else None
    data = random_input(rng, enc, 20000 + 3)
    want = M.stitched(data, enc, page, 4096)
    buf, n = _dev(data)
    torch.cuda.synchronize()
    assert U.transcode(buf.data_ptr(), n, enc, 0, page) == len(want)
    dst = torch.full((len(want) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(U.UgpuError) as e:
        U.transcode(buf.data_ptr(), n, enc, 0, page, dst.data_ptr(), len(want) - 1)
    assert e.value.code == 6 and e.value.out_len == len(want)
    assert bool(torch.all(dst == SENTINEL)), "UGPU_CAPACITY wrote"
    assert U.transcode(buf.data_ptr(), n, enc, 0, page, dst.data_ptr(), len(want)) == len(want)
    assert dst[:len(want)].cpu().numpy().tobytes() == want and bool(torch.all(dst[len(want):] == SENTINEL))


@pytest.mark.parametrize("enc", ENCS)
def test_tiny_inputs(U, enc):
    page = list(range(0x100, 0x200)) if enc == M.PAGE else None
    for data in (b"\xd8", b"\xd8\x00", b"\x00\xd8\x00", b"\xe9\x00\x00\x00", b"\x00\x00\x00\xe9\x0a", b"\n\x00\n\x00\n\x00\n"):
        _check(U, data, enc, M.direct(data, enc, page), (0, 1, 5), page)
    buf, n = _dev(b"abcd")
    assert _convert(U, buf, n, enc, 4, page) == (b"", 0)


# ---- boundaries

@pytest.mark.parametrize("enc", ENCS)
def test_sizes_around_tiles(U, enc):
    """k * 4096 + {0, 1, 2, 3, 5} bytes for k = 1 and 3: the last unit ends on
    the tile (and range) boundary, or a cut unit, one whole unit or a unit and
    a cut one lie behind it; the bytes behind the input are surrogates."""
    rng = np.random.default_rng(10 + enc)
    page = random_page(rng) if enc == M.PAGE else None
    for k in (1, 3):
        for extra in (0, 1, 2, 3, 5):
            data = random_input(rng, enc, k * 4096 + extra)
            if enc in U16:   # a high surrogate as the last whole unit
                m = len(data) // 2
                data = data[:2 * m - 2] + _units16(enc, [0xD800]) + data[2 * m:]
            _check(U, data, enc, M.stitched(data, enc, page, 4096), (0, 3), page)


@pytest.mark.parametrize("enc", U16)
def test_pairs_across_lanes_and_ranges(U, enc):
    """64 KiB + 6 bytes, every tile its own range.  A surrogate pair, then a
    lone H (with the unit it consumes), whose two units straddle a boundary B:
    a 64-byte lane boundary (B = 64 k inside a tile) and a wave-range boundary
    (B = 4096 k); and an H as the last unit before each, with a low surrogate
    two units on that must stay a lone one."""
    m = (64 << 10) // 2 + 3
    u = np.full(m, 0x61, np.int64)
    u[::37] = 0x20AC
    for i, b in enumerate(list(range(32, 2048, 32 * 5)) + list(range(2048, m - 8, 2048))):
        kind = i % 3
        u[b - 1] = 0xD800 + i
        u[b] = (0xDC00 + i, 0x41, 0xD900)[kind]       # a pair; H + BMP; H + H (the second H is consumed)
        u[b + 1] = (0x62, 0xDC00, 0xDC01)[kind]        # what follows is on its own
    data = _units16(enc, u)
    _check(U, data, enc, M.stitched(data, enc, None, 4096), (0, 2, 1))


@pytest.fixture(scope="module")
def big16():
    """(units, expected bytes) of the 32 MiB case, shared by both byte orders"""
    m = (32 << 20) // 2 + 3
    u = np.full(m, 0x61, np.int64)
    u[::101] = 0xE9
    u[7::4099] = 0x20AC
    bounds = list(range(2048, 64 * 2048, 2048)) + list(range(m - 64 * 2048 - 3, m - 8, 2048))
    for i, b in enumerate(bounds):
        b -= b % 2048
        if i % 4 == 3:
            run = 1 + i % 6
            u[b - run:b] = 0xD800 + i % 256
            u[b] = 0xDC00 if i % 8 == 3 else 0x7A
        else:
            u[b - 1] = 0xDB00 + i % 256
            u[b] = (0xDC00 + i % 256, 0x41, 0xD900)[i % 4]
            u[b + 1] = 0xDC02
    return u, M.stitched(_units16(M.UTF16LE, u), M.UTF16LE, None, 1 << 26)


@pytest.mark.parametrize("enc", U16)
def test_pairs_across_tiles_inside_a_range(U, big16, enc):
    """32 MiB + 6 bytes: 8193 tiles, so line_wave_ranges gives every wave two
    tiles or more and most 4 KiB boundaries lie inside a range.  A pair or a
    lone H straddles every 4 KiB boundary of the first 256 KiB and of the last,
    and H runs of 1 to 6 units end on further ones."""
    u, want = big16
    _check(U, _units16(enc, u), enc, want)


@pytest.mark.parametrize("enc", U16)
@pytest.mark.parametrize("odd", [0, 1])
def test_high_surrogates_throughout(U, enc, odd):
    """D800 through three whole ranges and a bit (an even and an odd count),
    then DC00 and 0041: the XOR carry through whole ranges."""
    data = _units16(enc, [0xD800] * (3 * 2048 + 40 + odd) + [0xDC00, 0x41])
    want = M.direct(data, enc)
    assert want.endswith(b"\xf0\x90\x80\x80A" if odd else M.NONCHAR * 2 + b"A")
    _check(U, data, enc, want, (0, 2))
    for tail in ([], [0xD800], [0x41, 0x42]):
        data = _units16(enc, [0x41] * odd + [0xD800] * (4 * 2048) + tail)
        _check(U, data, enc, M.direct(data, enc))


@pytest.mark.parametrize("enc", U16)
@pytest.mark.parametrize("kind", [0xE9, 0x20AC, 0xDC00])
def test_characters_across_destination_rows(U, enc, kind):
    """2-, 3- and 5-byte outputs from every offset 0..15: they straddle the
    16-byte rows of the destination, and the first row of the second and third
    range begins inside one (each range holds 2048 units)."""
    for pad in range(16):
        data = _units16(enc, [0x61] * pad + [kind] * (2 * 2048 + 100))
        _check(U, data, enc, M.direct(data, enc))


def test_short_last_range(U):
    """A last range of one to three units behind a whole one: its few output
    bytes begin at every offset of a destination row and end inside that row
    or the next, so no whole row of it is stored."""
    for enc in U16:
        for k in range(16):
            for tail in ([0x41], [0xE9, 0x41], [0x20AC], [0xDC00, 0x41, 0x42], [0xD800]):
                data = _units16(enc, [0xE9] * k + [0x61] * (2048 - k) + tail)
                _check(U, data, enc, M.direct(data, enc))
    for k in range(0, 16, 3):
        data = b"\xe9" * k + b"a" * (4096 - k) + b"\xe9b"
        _check(U, data, M.LATIN1, M.direct(data, M.LATIN1), (0, 1))


# ---- random inputs

@pytest.mark.parametrize("enc", ENCS)
def test_random_inputs(U, enc):
    rng = np.random.default_rng(1000 + enc)
    page = random_page(rng) if enc == M.PAGE else None
    n = ((1 << 20) if enc in U16 else (64 << 10) * (1 + enc % 3)) + 3
    data = random_input(rng, enc, n)
    want = M.stitched(data, enc, page, 1 << 16)
    buf, n = _dev(data, 2)
    first, _ = _convert(U, buf, n, enc, 2, page)
    second, _ = _convert(U, buf, n, enc, 2, page)
    assert first == second, "two runs differ"
    _check(U, data, enc, want, (2,), page)


# ---- end to end

FILES = (("lorem.utf16.txt", None), ("lorem.utf32.txt", None), ("lorem.latin1.txt", "latin1"))


@pytest.mark.parametrize("name,encoding", FILES)
def test_find_encoded_words(U, golden, name, encoding):
    import os
    _, g = golden
    data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify", name), "rb").read()
    rows = np.asarray(g["words"][name]["rows"], np.int64)
    assert len(rows) == 1283
    r = U.find_encoded(U.Pattern(U.compile_regex(r"\w+")), data, encoding)
    assert r.count == len(rows)
    assert np.array_equal(r.start.astype(np.int64), rows[:, 0]) and np.array_equal(r.length.astype(np.int64), rows[:, 1])
    # -iwco -f lorem
    pats = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify", "lorem"), "rb").read()
    rx = "|".join(pats.decode().split())
    pat = U.Pattern(U.compile_regex(rx, icase=True), word=True)
    assert g["words"][name]["iwco"] == 18
    assert U.find_encoded(pat, data, encoding, offsets=False).count == 18


def test_decode_input(U):
    text = "día ünö €\n".encode()
    for data, kw in ((b"\xef\xbb\xbf" + text, {}), (text, {}), (b"\xff\xfe" + text.decode().encode("utf-16-le"), {}),
                     (b"\xfe\xff" + text.decode().encode("utf-16-be"), {}),
                     (text.decode().encode("utf-32-le"), dict(encoding="utf-32le")),
                     (text.decode().encode("cp1252"), dict(page=[ord(bytes([b]).decode("cp1252", "replace")) for b in range(256)]))):
        dev, n = U.decode_input(data, **kw)
        assert dev.data_ptr() % 16 == 0 and dev.numel() >= n + 16 and dev[:n].cpu().numpy().tobytes() == text
        assert not bool(dev[n:].any())
    dev, n = U.decode_input(b"a\x00b\nc", encoding="null-data")
    assert dev[:n].cpu().numpy().tobytes() == b"a\nb\x00c"


# ---- outputs past 2^32

def test_output_past_4gib(U):
    """2.2 GiB of Latin-1 0xE9 with a few ASCII bytes, so that the two-byte
    characters behind them lie at odd output offsets: the output passes 2^32.
    The length, and the bytes around the output offsets 2^31, 2^32 and the end,
    from the model over the input bytes that give them."""
    n = (2252 << 20) + 5
    ascii_at = [5, (1 << 30) + 1, (1 << 31) + 77, n - 3]
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    buf.fill_(0xE9)
    for p in ascii_at:
        buf[p] = 0x78
    torch.cuda.synchronize()
    m = U.transcode(buf.data_ptr(), n, M.LATIN1)
    assert m == 2 * n - len(ascii_at) > (1 << 32)
    dst = torch.empty(m + 64, dtype=torch.uint8, device="cuda")
    dst[m:] = SENTINEL
    torch.cuda.synchronize()
    assert U.transcode(buf.data_ptr(), n, M.LATIN1, 0, None, dst.data_ptr(), m) == m
    assert bool(torch.all(dst[m:] == SENTINEL))

    def out_offset(i):
        return 2 * i - sum(1 for p in ascii_at if p < i)

    for centre in (300, (1 << 30), (1 << 31) + 77, n - 300):
        i0, i1 = centre - 300, min(centre + 300, n)
        want = M.direct(buf[i0:i1].cpu().numpy().tobytes(), M.LATIN1)
        at = out_offset(i0)
        assert dst[at:at + len(want)].cpu().numpy().tobytes() == want, centre
    at = out_offset((1 << 31) + 77 - 300)
    assert at < (1 << 32) - 64 and at + 1100 > (1 << 32) + 64        # that window holds output offset 2^32
    assert out_offset((1 << 30) - 300) < (1 << 31) < out_offset((1 << 30) + 300)
    assert dst[m - 1].item() == 0xA9
    del buf, dst
    torch.cuda.empty_cache()
