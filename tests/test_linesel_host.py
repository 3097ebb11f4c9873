"""CPU: the host half of the line records (ugrep_amd.context_lines) against a
brute-force mask model, and the numpy model of the selection semantics
(tests/linesel_model.py) against the reference's recorded CLI outputs
(tests/golden/linesel_cases.json, from tests/out/Hello_*{-n,-nv,-nC2,-nvC2}.out):
the second guards the fixture and the model the GPU tests compare with."""
import json
import os

import numpy as np
import pytest

import linesel_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def linesel():
    with open(os.path.join(GOLDEN, "linesel_cases.json")) as f:
        return json.load(f)


def _data(name):
    return np.frombuffer(open(os.path.join(GOLDEN, "verify", name), "rb").read(), np.uint8)


@pytest.mark.parametrize("before", [0, 1, 2, 7])
@pytest.mark.parametrize("after", [0, 1, 2, 7])
def test_context_lines_vs_sets(before, after):
    from ugrep_amd import context_lines
    rng = np.random.default_rng(100 * before + after)
    sels = [[], [1], [40], [1, 40], [1, 2, 3], [5, 7], [5, 6 + before + after], [5, 7 + before + after],
            [38, 39, 40], list(range(1, 41))]
    for dens in (0.02, 0.1, 0.5):
        sels.append((np.flatnonzero(rng.random(40) < dens) + 1).tolist())
    for sel in sels:
        lineno, kind = context_lines(np.asarray(sel, np.uint64), 40, before, after)
        want = M.context_sets(sel, 40, before, after)
        assert lineno.tolist() == want[0], (sel, before, after)
        assert kind.tolist() == want[1], (sel, before, after)
    big = np.flatnonzero(rng.random(5000) < 0.01) + 1
    lineno, kind = context_lines(big, 5000, before, after)
    want = M.context_sets(big, 5000, before, after)
    assert lineno.tolist() == want[0] and kind.tolist() == want[1]


def test_model_reproduces_reference_outputs(linesel):
    opts = {"-n": (False, 0), "-nv": (True, 0), "-nC2": (False, 2), "-nvC2": (True, 2)}
    seen = 0
    for c in linesel["cases"]:
        data = _data(c["file"])
        m = np.asarray(c["matches"], np.int64).reshape(-1, 2)
        for opt, want in c["printed"].items():
            inv, ctx = opts[opt]
            lineno, kind, begin, end = M.grep(data, m[:, 0], m[:, 1], inv, ctx, ctx)
            assert [list(x) for x in zip(lineno, kind)] == want, (c["file"], c["pattern"], opt)
            seen += 1
        if "counts" in c:
            assert M.select(data, m[:, 0], m[:, 1])[2].size == c["counts"]["-c"], (c["file"], c["pattern"])
            assert cv_count(M.select(data, m[:, 0], m[:, 1], True), len(data)) == c["counts"]["-cv"], \
                (c["file"], c["pattern"])
    assert seen == 96 + 6


def cv_count(records, n):
    """ugrep -cv from the inverted records: the reference computes it as the
    newline count minus the -c count (src/ugrep.cpp:10625-10631), so an
    unterminated last line, which -nv prints (Hello.txt: -nv prints line 1, -cv
    says 0), is not counted: count the records that end on a newline."""
    return int(np.count_nonzero(records[1] < n))


def test_model_line_table():
    for raw, want in ((b"", []), (b"a\n", [(0, 1)]), (b"a", [(0, 1)]), (b"\n", [(0, 0)]), (b"a\n\nbc", [(0, 1), (2, 2), (3, 5)])):
        b, e = M.line_table(np.frombuffer(raw, np.uint8))
        assert list(zip(b.tolist(), e.tolist())) == want, raw
