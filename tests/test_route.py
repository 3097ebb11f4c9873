"""The kernel route of a scan (plan.hpp dfa_route; DESIGN "kernel routes").

CPU: the host plan over patterns x options x test knobs equals
tests/golden/route_cases.json, the project's own output recorded before the
route was gathered into one function (tests/golden/make_route_golden.py).

GPU: one child process (tests/route_child.py) runs every case with
UGPU_TRACE=1.  The first step of a scan runs the kernel Pattern.info() reports;
each of the four redo rules leads through the expected steps and no further;
OFFSETS after an xi_kernel COUNT recounts and writes on dense_kernel.  All
results equal the oracle restatement."""
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_route_golden  # noqa: E402

WFAST = 16  # UGPU_TOT_WFAST


def test_route_equals_golden():
    with open(make_route_golden.OUT) as f:
        want = json.load(f)["settings"]
    assert sorted(want) == sorted(k or "none" for k in make_route_golden.SETTINGS)
    with ThreadPoolExecutor(len(make_route_golden.SETTINGS)) as ex:  # (one child process per knob setting)
        got = list(ex.map(make_route_golden.run_setting, make_route_golden.SETTINGS))
    for knob, cases in zip(make_route_golden.SETTINGS, got):
        w = want[knob or "none"]
        assert sorted(cases) == sorted(w), knob
        for key in w:
            assert cases[key] == w[key], (knob, key)


_SCAN = re.compile(r"^\[ugpu\] scan .* kernel (\d)( w)?( edge)?( exact)?$")
_OFFS = re.compile(r"^\[ugpu\] offsets (recount|write) kernel (\d)$")


def parse_trace(text):
    """{case: [step, ...]}: "6", "6 exact", "6 edge", "5 w", and "recount 1" /
    "write 1" for the passes of ugpu_scan_offsets"""
    steps, cur = {}, None
    for line in text.split("\n"):
        if line.startswith("[case] "):
            cur = steps.setdefault(line[7:], [])
        elif line.startswith("[ugpu] scan "):
            m = _SCAN.match(line)
            assert m, line
            cur.append(m.group(1) + "".join(g or "" for g in m.groups()[1:]))
        elif line.startswith("[ugpu] offsets "):
            m = _OFFS.match(line)
            if m:
                cur.append("%s %s" % m.groups())
    return steps


@pytest.fixture(scope="module")
def child():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    env = {k: v for k, v in os.environ.items() if k not in make_route_golden.ALL_KNOBS + ["UGPU_MAX_GRID"]}
    env["UGPU_TRACE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "route_child.py")], env=env, capture_output=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout.decode().strip().split("\n")[-1]), parse_trace(r.stderr.decode())


@pytest.mark.gpu
def test_results_equal_oracle(child):
    out, steps = child
    assert len(out) == 2 * 12 + 8 + 1
    for name, c in out.items():
        assert c["got"] == c["want"], name
        assert steps[name], name


@pytest.mark.gpu
def test_first_step_is_the_reported_kernel(child):
    out, steps = child
    first = [n for n in out if n.startswith("first|")]
    assert len(first) == 24
    for name in first:
        assert int(steps[name][0][0]) == out[name]["kernel"], (name, steps[name])
    # (every kernel number is among them)
    assert {out[n]["kernel"] for n in first} >= {0, 2, 4, 5, 6, 7}


# case -> (steps, UGPU_TOT_WFAST in the totals' flags; None: not an option-W fast path)
REDO = {
    "redo|w+|clean": (["6"], None),
    "redo|w+|mixed": (["6", "6 exact"], None),
    "redo|w+|mixed again": (["6 exact"], None),  # (the exact U kernel until the scanner goes back to its pool)
    "redo|w+|four": (["6", "6 exact", "3"], None),
    "redo|-w w+|clean": (["6 edge"], True),
    "redo|-w w+|stray": (["6 edge", "4 w"], False),
    "redo|-w ident|ascii": (["5 w"], True),
    "redo|-w ident|high": (["5 w", "4 w"], False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REDO))
def test_redo_steps(child, name):
    out, steps = child
    want, wfast = REDO[name]
    assert steps[name] == want
    assert bool(out[name]["flags"] & WFAST) == bool(wfast)


@pytest.mark.gpu
def test_offsets_after_xi_count(child):
    out, steps = child
    assert out["offsets|ident"]["kernel"] == 2
    assert steps["offsets|ident"] == ["2", "recount 1", "write 1"]
