"""The sparse kernel's two-field prefilter (tables.hpp filter2, sparse_kernel.hip
bucket_bits<true>): the lookup on a byte's top two bits is left out, so a byte
also passes for its aliases in the other 64-byte quadrants (`f` and `&`).

CPU: the two-field candidates contain the three-field ones, which contain every
match start; the host chooses the form by the candidate density it adds
(kFilter2Added) and reports it as UGPU_SHAPE_FILTER2.
GPU: scans under the two-field form equal the oracle and the same scan under
UGPU_FT2=0, record by record -- at lane, chunk and tile edges, at the end of
final and non-final ranges, on alias-dense input, forced on for a table the
rule refuses, and through the STAGE / WRITE instantiations."""
import itertools
import os
import re

import numpy as np
import pytest

import ugrep_amd
from ugrep_amd import _lib
from oracle_lib import OracleDfa, case_input, gen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = [10] + list(range(0x20, 0x7f))


# ------------------------------------------------------------------ the model
def _bits3(ft, b):
    return ft[b & 7] & ft[8 + ((b >> 3) & 7)] & ft[16 + (b >> 6)]


def _bits2(ft, b):
    return ft[b & 7] & ft[8 + ((b >> 3) & 7)]


def _hit(R0, R1, R2):
    return any((R0 >> g) & 1 and (R1 >> (2 + g)) & 1 and (R2 >> (4 + g)) & 1 for g in (0, 1))


def _candidates(bits, ft, data):
    R = [bits(ft, b) for b in data] + [0x3F, 0x3F]
    return {i for i in range(len(data)) if _hit(R[i], R[i + 1], R[i + 2])}


def _density(bits, ft, alphabet):
    """Sum over the two groups of the product of their three sets' fractions of
    the alphabet (tables.cpp Lead::density and its two-field / uniform forms)."""
    d = 0.0
    for g in (0, 1):
        f = 1.0
        for s in range(3):
            f *= sum((bits(ft, b) >> (2 * s + g)) & 1 for b in alphabet) / len(alphabet)
        d += f
    return min(1.0, d)


def _added(ft):
    """Candidate density the two-field form adds: (on text, on uniform bytes)."""
    return (_density(_bits2, ft, TEXT) - _density(_bits3, ft, TEXT),
            _density(_bits2, ft, range(256)) - _density(_bits3, ft, range(256)))


def _bound():
    src = open(os.path.join(REPO, "ugrep_amd", "csrc", "tables.hpp")).read()
    return float(re.search(r"constexpr double kFilter2Added = ([0-9.eE+-]+);", src).group(1))


def test_two_field_candidates_are_a_superset(patterns, cases):
    seen = set()
    for c in cases:
        if c["matches"] is None or c["input"]["type"] != "hex":
            continue
        try:
            enabled, ft = ugrep_amd.host_prefilter(patterns[c["pattern"]]["opc"])
        except ugrep_amd.Unsupported:
            continue
        if not enabled:
            continue
        seen.add(c["pattern"])
        ft, data = ft.tolist(), case_input(c["input"]).tolist()
        c3, c2 = _candidates(_bits3, ft, data), _candidates(_bits2, ft, data)
        assert c3 <= c2, (c["pattern"], c["input"].get("name"))
        assert {m[0] for m in c["matches"]} <= c3, (c["pattern"], c["input"].get("name"))
    assert {"c1_lorem", "c2_foobarbaz", "hello"} <= seen


def test_two_field_selectivity_c2(patterns):
    enabled, ft = ugrep_amd.host_prefilter(patterns["c2_foobarbaz"]["opc"])
    assert enabled
    ft = ft.tolist()
    R = {b: _bits2(ft, b) for b in range(256)}
    assert all(r < 0x40 for r in R.values())  # bits 6, 7 stay 0 (cand_flags relies on it)
    passed = {bytes(t) for t in itertools.product(TEXT, repeat=3) if _hit(R[t[0]], R[t[1]], R[t[2]])}
    want = {bytes(t) for t in itertools.product(b"f&", b"o/", b"o/")}
    want |= {bytes(t) for t in itertools.product(b'b"', b"a!", b"rz2:")}
    assert len(want) == 24 and passed == want


def _filter2(opc):
    return bool(ugrep_amd.host_plan(opc)["shape"] & _lib.SHAPE_FILTER2)


def test_host_chooses_the_form(patterns, monkeypatch):
    monkeypatch.delenv("UGPU_FT2", raising=False)
    assert _filter2(ugrep_amd.compile_regex("foo|bar|baz"))
    assert _filter2(ugrep_amd.compile_regex("lorem", fixed=True))
    assert not _filter2(patterns["c3_ident"]["opc"])             # dense
    assert not _filter2(ugrep_amd.compile_regex("[a-z]+ing"))    # loop needle: three fields
    assert not bool(ugrep_amd.host_plan(ugrep_amd.compile_regex("foo|bar|baz"), word=True)["shape"]
                    & _lib.SHAPE_FILTER2)                        # option W: three fields
    # sparse patterns on both sides of the bound, judged by the model above
    bound, refused = _bound(), 0
    for rx in ("[a-h]b[a-h]", "[a-p][a-p]x", "[a-c]x[a-c]", "hello", "the|then", "[xyz]q[0-9]"):
        opc = ugrep_amd.compile_regex(rx)
        enabled, ft = ugrep_amd.host_prefilter(opc)
        assert enabled, rx
        assert ugrep_amd.host_plan(opc)["kernel"] == 0, rx
        at, au = _added(ft.tolist())
        assert abs(at - bound) > 1e-9 and abs(au - bound) > 1e-9, rx  # (no tie with the bound)
        want = at <= bound and au <= bound
        assert _filter2(opc) == want, (rx, at, au, bound)
        refused += not want
    assert refused >= 1
    # UGPU_FT2 forces the form off / on for tables on the plain sparse path only
    monkeypatch.setenv("UGPU_FT2", "0")
    assert not _filter2(ugrep_amd.compile_regex("foo|bar|baz"))
    monkeypatch.setenv("UGPU_FT2", "1")
    assert _filter2(ugrep_amd.compile_regex("[a-h]b[a-h]"))
    assert not _filter2(patterns["c3_ident"]["opc"])
    assert not _filter2(ugrep_amd.compile_regex("[a-z]+ing"))


# ------------------------------------------------------------------------ GPU
REFUSED = "[a-h]b[a-h]"  # (test_host_chooses_the_form: the rule refuses it)
TRIGRAMS = [b"foo", b"bar", b"baz", b"&//", b'"!2', b'"!:', b"\xe6\xaf\xef", b"\xa2\xe1\xfa", b"f/o", b'"a:',
            b"\xe6oo", b"ba\xb2"]


@pytest.fixture(scope="module")
def G():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch


def _scan(G, pat, dev, hi, read_end, at_eof, ft2, records=False, stage=None):
    """(count, digest, dcap, exit, flags) and the OFFSETS records of dev[0:hi)
    under UGPU_FT2=ft2."""
    st = G.cuda.current_stream().cuda_stream
    os.environ["UGPU_FT2"] = str(ft2)
    try:
        sc = ugrep_amd.Scanner(pat, records=records)
        if stage is not None:
            sc.stage(stage)
        sc.scan(dev.data_ptr(), 0, hi, read_end, at_eof, 0, st)
        t = sc.totals()
        cnt = t.count
        s = G.empty(max(cnt, 1), dtype=G.int64, device="cuda")
        ln = G.empty(max(cnt, 1), dtype=G.int32, device="cuda")
        cp = G.empty(max(cnt, 1), dtype=G.int32, device="cuda")
        sc.offsets(s.data_ptr(), ln.data_ptr(), cp.data_ptr(), cnt, st)
        G.cuda.synchronize()
        sc.close()
    finally:
        os.environ.pop("UGPU_FT2", None)
    recs = [list(r) for r in zip(s[:cnt].cpu().tolist(), ln[:cnt].cpu().tolist(), cp[:cnt].cpu().tolist())]
    return (t.count, t.digest, t.dcap, t.exit, t.flags & 7), recs


def _expect(opc, host, hi):
    """The oracle's totals and records of the matches of host that start below hi."""
    cnt, dg, dc, lst = OracleDfa(opc).find(host, want_list=True)
    lst = [r for r in lst if r[0] < hi]
    M = 1 << 64
    end = lst[-1][0] + lst[-1][1] if lst else hi
    return (len(lst), sum(s * 31 + l for s, l, _ in lst) % M, sum((s + 1) * c for s, _, c in lst) % M,
            max(end, hi), 0), lst


def _both_forms(G, opc, host, hi, at_eof, **kw):
    pat = ugrep_amd.Pattern(opc)
    assert pat.info()["kernel"] == 0
    dev = G.from_numpy(host).to("cuda")
    want = _expect(opc, host, hi)
    got2 = _scan(G, pat, dev, hi, host.size, at_eof, 1, **kw)
    got3 = _scan(G, pat, dev, hi, host.size, at_eof, 0, **kw)
    assert got2[0] == want[0] and got3[0] == want[0], (got2[0], got3[0], want[0])
    assert got2[1] == want[1]
    assert got3[1] == want[1]
    return want


def _edge_buffer(n, halo, rot):
    """n + halo bytes of word text with needles and alias trigrams that start at
    offsets 13-16 of a lane's 16 bytes, in the last three bytes before every
    chunk (1 KiB) and tile (4 KiB) edge and on it, and in the last three bytes
    of the range; `rot` rotates trigrams and offsets so that the sizes together
    cover every pairing."""
    host = gen(1, 40 + rot, 0, n + halo).copy()
    spots = [96 * (j + 1) + 13 + (j + rot) % 4 for j in range(8)]
    spots += [1024 * m - (m + rot) % 4 for m in range(1, n // 1024 + 1)]
    spots += [n - 3 + rot % 3]
    end = 0
    for k, p in enumerate(sorted(set(spots))):
        tri = TRIGRAMS[(k + rot) % len(TRIGRAMS)]
        if p < end or p >= n:
            continue
        m = min(3, n + halo - p)
        host[p:p + m] = np.frombuffer(tri[:m], np.uint8)
        end = p + 3
    return host


SIZES = [4096 * t + d for t in (1, 2, 3) for d in (0, 1, 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("halo", [0, 32], ids=["eof", "halo"])
@pytest.mark.parametrize("n", SIZES)
def test_edges(G, patterns, n, halo):
    opc = patterns["c2_foobarbaz"]["opc"]
    for rot in (SIZES.index(n), SIZES.index(n) + 5):
        host = _edge_buffer(n, halo, rot)
        want = _both_forms(G, opc, host, n, halo == 0)
        assert want[0][0] >= 2  # (needles were planted)


@pytest.mark.gpu
def test_alias_dense(G, patterns):
    opc = patterns["c2_foobarbaz"]["opc"]
    n = 256 << 10
    host = np.frombuffer((b"&//" * (n // 3 + 1))[:n], np.uint8).copy()
    enabled, ft = ugrep_amd.host_prefilter(opc)
    ft = ft.tolist()
    head = host[:3000].tolist()
    assert not _candidates(_bits3, ft, head)
    assert {i for i in _candidates(_bits2, ft, head) if i < 2997} == set(range(0, 2997, 3))
    want = _both_forms(G, opc, host, n, True)
    assert want[0] == (0, 0, 0, n, 0)  # no match, no error flag
    host[np.arange(5, n - 3, 4099)[:, None] + np.arange(3)] = np.frombuffer(b"foo", np.uint8)
    want = _both_forms(G, opc, host, n, True)
    assert want[0][0] == len(range(5, n - 3, 4099))


@pytest.mark.gpu
def test_forced_on_for_a_refused_table(G):
    opc = ugrep_amd.compile_regex(REFUSED)
    assert not _filter2(opc)
    os.environ["UGPU_FT2"] = "1"
    try:
        assert ugrep_amd.Pattern(opc).info()["shape"] & _lib.SHAPE_FILTER2
    finally:
        os.environ.pop("UGPU_FT2", None)
    want = _both_forms(G, opc, gen(1, 9, 0, 64 << 10).copy(), 64 << 10, True)
    assert want[0][0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [True, False], ids=["staged", "write"])
def test_several_waves_records(G, patterns, stage):
    opc = patterns["c2_foobarbaz"]["opc"]
    assert ugrep_amd.Pattern(opc).info()["shape"] & _lib.SHAPE_FILTER2
    host = gen(1, 12, 0, 1 << 20).copy()
    host[np.arange(4094, host.size - 3, 4096)[:, None] + np.arange(3)] = np.frombuffer(b"bar", np.uint8)
    host[777:780] = np.frombuffer(b"&//", np.uint8)
    want = _both_forms(G, opc, host, host.size, True, records=True, stage=stage)
    assert want[0][0] > 255
