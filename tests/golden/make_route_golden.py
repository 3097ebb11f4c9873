#!/usr/bin/env python3
"""Generate tests/golden/route_cases.json: the project's own host plan
(ugrep_amd.host_plan: table shape, prefilter estimate and the kernel of a COUNT
scan) over patterns x options W, N x the kernel-choice test knobs.  The file
pins the routing decision: it was recorded before the route was gathered into
one function (plan.hpp dfa_route), and tests/test_route.py asserts that the
build reproduces it exactly.

The knobs are read from the environment by the host library, so one child
process runs per knob setting (this file with --child) and prints its cases as
one JSON line.  A case that the plan rejects is recorded as "unsupported".

No device and no reference sources are needed; the output is data, committed."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "route_cases.json")

KNOBS = ["UGPU_SPARSE", "UGPU_XI", "UGPU_XG", "UGPU_XC", "UGPU_XU", "UGPU_NG", "UGPU_WFAST", "UGPU_WSPARSE",
         "UGPU_LB"]
# every knob that moves the plan or the route (a caller's setting must not leak into a child)
ALL_KNOBS = KNOBS + ["UGPU_XUW", "UGPU_FT2"]
SETTINGS = [None] + KNOBS  # no knob, then each knob = 0 alone


def patterns():
    """[(name, regex)]: tests/test_plan.py's list, context and loop-needle
    tables, lookahead, two string sets (class and wide n-gram tables) and a
    wide table."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import test_plan
    import wordset_gen
    pats = [(rx, rx) for rx in test_plan.PATS]
    pats += [(rx, rx) for rx in (r"\bfoo\b", r"\<(in|ut)\>", "[a-z]+(ing|ed)", "foo(?=bar)")]
    pats.append(("words300", wordset_gen.regex(wordset_gen.words(300))))
    pats.append(("words3000", wordset_gen.regex(wordset_gen.words(3000))))
    pats.append((r"\w+ \w+", r"\w+ \w+"))  # (tests/test_wide.py: more than 64 Ki table entries)
    return pats


def child():
    sys.path.insert(0, REPO)
    import ugrep_amd as U
    out = {}
    for name, rx in patterns():
        try:
            opc = U.compile_regex(rx)
        except U.Unsupported:
            out[name] = "unsupported"
            continue
        for word in (False, True):
            for empty in (False, True):
                key = "%s|w%d|n%d" % (name, word, empty)
                try:
                    out[key] = U.host_plan(opc, word=word, empty=empty)
                except U.Unsupported:
                    out[key] = "unsupported"
    print(json.dumps(out, sort_keys=True))


def run_setting(knob):
    """The cases of one knob setting (knob = "0", or no knob), from a child process."""
    env = {k: v for k, v in os.environ.items() if k not in ALL_KNOBS}
    if knob:
        env[knob] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True)
    if r.returncode:
        raise RuntimeError("route child failed (%s): %s" % (knob, r.stderr.decode()[-400:]))
    return json.loads(r.stdout.decode().strip().split("\n")[-1])


def main():
    doc = {"settings": {knob or "none": run_setting(knob) for knob in SETTINGS}}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
    n = sum(len(v) for v in doc["settings"].values())
    print("%d cases -> %s (%d bytes)" % (n, OUT, os.path.getsize(OUT)), file=sys.stderr)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
