"""CPU: Boolean line queries (ugpu_select_lines_bool, include/ugpu.h).  The
numpy model (tests/boolsel_model.py) reproduces what the reference CLI prints
for its own --bool suite (tests/golden/boolsel_cases.json) from the recorded
sub-pattern match lists; parse_bool_query normalises those queries to the CNF
written by hand here; ugpu_tables_newline_host tells which tables can match a
newline."""
import json
import os

import numpy as np
import pytest

import boolsel_model as B
import ugrep_amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MODES = {"-n": (False, 0), "-n --files": (True, 0), "-nC2": (False, 2), "-nC2 --files": (True, 2)}

# the ten queries of the reference's CLI suite (tests/verify.sh:354) and their
# CNF: patterns in order of first appearance, one (pos, neg) mask pair per clause
CNF = [
    ("", [], []),
    ("Hello World", ["Hello", "World"], [(1, 0), (2, 0)]),
    ("Hello -World", ["Hello", "World"], [(1, 0), (0, 2)]),
    ("Hello -bin", ["Hello", "bin"], [(1, 0), (0, 2)]),
    ("bin -Hello", ["bin", "Hello"], [(1, 0), (0, 2)]),
    ("bin -greeting", ["bin", "greeting"], [(1, 0), (0, 2)]),
    ("Hello -World|greeting", ["Hello", "World", "greeting"], [(1, 0), (4, 2)]),      # Hello & (!World | greeting)
    ("Hello -bin|greeting", ["Hello", "bin", "greeting"], [(1, 0), (4, 2)]),
    ("Hello -(greeting|World)", ["Hello", "greeting", "World"], [(1, 0), (0, 2), (0, 4)]),  # Hello & !greeting & !World
    ('"a Hello" greeting', ["\\Qa Hello\\E", "greeting"], [(1, 0), (2, 0)]),
]


@pytest.fixture(scope="module")
def boolsel():
    with open(os.path.join(GOLDEN, "boolsel_cases.json")) as f:
        return json.load(f)


def _file(name):
    return np.frombuffer(open(os.path.join(GOLDEN, "verify", name), "rb").read(), np.uint8)


def case_lists(c):
    out = []
    for m in c["matches"]:
        m = np.asarray(m, np.int64).reshape(-1, 2)
        out.append((m[:, 0], m[:, 1]))
    return out


def test_model_reproduces_reference_cases(boolsel):
    assert len(boolsel["cases"]) == 13 * 6
    nonempty = 0
    for c in boolsel["cases"]:
        data = _file(c["file"])
        clauses = [tuple(x) for x in c["clauses"]]
        for mode, (files, ctx) in MODES.items():
            got = B.grep(data, case_lists(c), clauses, False, files, ctx, ctx)
            assert got == c["printed"][mode], (c["query"], c["file"], mode)
            nonempty += bool(got)
    assert nonempty > 100


def test_parse_reference_queries(boolsel):
    for q, patterns, clauses in CNF:
        assert ugrep_amd.parse_bool_query(q) == (patterns, clauses), q
    # the generator's hand-written CNF of the same queries agrees
    seen = {c["query"]: (c["patterns"], [tuple(x) for x in c["clauses"]]) for c in boolsel["cases"] if c["bool"]}
    assert seen == {q: (p, cl) for q, p, cl in CNF}


def test_parse_grammar():
    P = ugrep_amd.parse_bool_query
    assert P("A AND B") == P("A B") == (["A", "B"], [(1, 0), (2, 0)])
    assert P("A OR B") == P("A|B") == P("A || B") == (["A", "B"], [(3, 0)])
    assert P("NOT A") == P("-A") == P("- A") == (["A"], [(0, 1)])
    assert P("A B|C -D") == (["A", "B", "C", "D"], [(1, 0), (6, 0), (0, 8)])
    # NOT binds tighter than OR, OR tighter than AND; De Morgan; distribution
    assert P("-(A B)") == (["A", "B"], [(0, 3)])
    assert P("-(A|B)") == (["A", "B"], [(0, 1), (0, 2)])
    assert P("A|(B C)") == (["A", "B", "C"], [(3, 0), (5, 0)])
    assert P("(A B)|(C D)") == (["A", "B", "C", "D"], [(5, 0), (9, 0), (6, 0), (10, 0)])
    assert P("A|-A B") == (["A", "B"], [(2, 0)])                       # a true clause is dropped
    assert P("A B A") == (["A", "B"], [(1, 0), (2, 0)])                # equal patterns share a list
    # a '(' that is part of a regex, brackets, escapes and quotes do not split a pattern
    assert P("(foo|bar)? x") == (["(foo|bar)?", "x"], [(1, 0), (2, 0)])
    assert P("(?i:a|b) c") == (["(?i:a|b)", "c"], [(1, 0), (2, 0)])
    assert P("[a |b] c") == (["[a |b]", "c"], [(1, 0), (2, 0)])
    assert P(r"a\ b c\|d") == ([r"a\ b", r"c\|d"], [(1, 0), (2, 0)])
    assert P('"a|b (c" d') == (["\\Qa|b (c\\E", "d"], [(1, 0), (2, 0)])
    assert P('x"y z"') == (["x\\Qy z\\E"], [(1, 0)])
    assert P("ANDY ORB NOTE") == (["ANDY", "ORB", "NOTE"], [(1, 0), (2, 0), (4, 0)])


def test_parse_limits():
    P = ugrep_amd.parse_bool_query
    names = ["p%02d" % i for i in range(17)]
    assert len(P(" ".join(names[:16]))[0]) == 16
    with pytest.raises(ValueError):
        P(" ".join(names))                       # 17 distinct patterns
    with pytest.raises(ValueError):
        P("|".join(names))
    assert len(P("(a b)|(c d)|(e f)|(g h)|(i j)|(k l)")[1]) == 64
    with pytest.raises(ValueError):
        P("(a b)|(c d)|(e f)|(g h)|(i j)|(k l)|(m n)")   # 128 clauses
    for bad in ("a )", "(a b", "a | | b x )", "()", 'a ""', "a\nb"):
        with pytest.raises(ValueError):
            P(bad)


def test_tables_newline_host():
    """The table decides, not the regex text: under ugrep's conversion
    (compile_regex's default, convert_flag::notnewline) \\s and [^a] leave the
    newline out; as plain RE/flex regexes they hold it."""
    nl = ugrep_amd.host_newline
    C = ugrep_amd.compile_regex
    for rx in ("Hello", "[a-z]+"):
        assert nl(C(rx, reflex=True)) is False and nl(C(rx)) is False, rx
    for rx in (r"\S\n\S", r"\s+", "[^a]"):
        assert nl(C(rx, reflex=True)) is True, rx
    assert nl(C(r"\S\n\S")) is True
    assert nl(C(r"\s+")) is False and nl(C("[^a]")) is False
    for rx in ("^Hello$", r"\bHello\b", "a$"):   # anchors consume no byte
        assert nl(C(rx)) is False, rx
    from ugrep_amd import _lib
    with pytest.raises(ugrep_amd.UgpuError):
        _lib.check(_lib.lib.ugpu_tables_newline_host(None, 0, None))


def test_golden_patterns_compile_without_newline(boolsel):
    """What grep_bool does with each sub-pattern before it scans: \\Q...\\E spans
    become escaped characters for the native compiler, and no table of the
    reference suite can match a newline."""
    from ugrep_amd.matcher import _expand_quotes
    assert _expand_quotes("\\Qa Hello\\E") == "a Hello"
    assert _expand_quotes("x\\Qa.b|(c\\E\\\\E\\Q)\\Ey\\.") == "xa\\.b\\|\\(c\\\\E\\)y\\."
    for rx in sorted({p for c in boolsel["cases"] for p in c["patterns"]}):
        assert ugrep_amd.host_newline(ugrep_amd.compile_regex(_expand_quotes(rx))) is False, rx


def test_newline_host_on_recorded_tables(patterns):
    assert ugrep_amd.host_newline(patterns["hello"]["opc"]) is False
    assert ugrep_amd.host_newline(patterns["hello_wnhS"]["opc"]) is True   # \w+[\n\h]+\S+
