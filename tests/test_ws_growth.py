"""The growth paths of the pooled workspaces (hip_host.hpp HipBuf / WsLease; the
FindWs, RecWs and slot workspaces of engine.hip and utf8.hip).

The pools live as long as the process, so in the suite's own process whether a
buffer grows depends on what ran earlier.  One child process
(tests/ws_growth_child.py) starts from empty pools and walks through: find_all
inputs that outgrow the input copy and the record lists twice, a stream whose
buffers grow while it holds a carry, a batch served input by input whose record
lists grow while they hold records, two records calls, and the binary tests.
Every result equals the oracle restatement, record for record.

CPU: the oracle side of every step runs, each step's inputs are as large as the
growth they are meant to force, and the batch takes the per-input path
(host_batch_plan and the bare-CR rule decide that without a device)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ws_growth_child as child_mod
from oracle_lib import OracleDfa, first_nul, is_binary, utf8_first_bad

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def want():
    """The oracle's answer to every step of the child, computed once."""
    ins, tab = child_mod.inputs(), child_mod.tables()
    c2, c3, eol = OracleDfa(tab["c2"]), OracleDfa(tab["c3"]), OracleDfa(tab["eol"])
    whole = c2.find(ins["planted"], want_list=True)
    return dict(
        ins=ins, tab=tab,
        find_all=[list(c2.find(ins["planted"][:n], want_list=True)) for n in child_mod.FIND_SIZES],
        stream=[whole[0], whole[3]],
        batch=[list(eol.find(np.frombuffer(d, np.uint8), want_list=True)) for d in ins["batch"]],
        records=[list(c3.find(ins["code"][:n])[:3]) for n in child_mod.REC_SIZES],
        utf8=[dict(first_bad=utf8_first_bad(d), binary=is_binary(d), nul=first_nul(d)) for d in ins["utf8"]])


def test_inputs_force_the_growth(want):
    import ugrep_amd as U
    ins, tab = want["ins"], want["tab"]
    # 1. bytes and records both exceed 1.25x the step before: n + n/4 does not cover the next
    sizes, counts = child_mod.FIND_SIZES[:3], [w[0] for w in want["find_all"][:3]]
    for a, b in zip(sizes, sizes[1:]):
        assert b > a + a // 4
    for a, b in zip(counts, counts[1:]):
        assert a > 0 and b > a + a // 4
    assert want["find_all"][3] == want["find_all"][0]
    # 2. the first two feeds settle nothing (a carry is held), the third passes the initial 1 MiB
    assert sum(child_mod.FEEDS[:2]) <= child_mod.KEEP and sum(child_mod.FEEDS) > 1 << 20
    assert want["stream"][0] > 0
    # 3. one scan would do but for the line context and the bare CR; the lists
    # outgrow what steps 1 and 2 left (their largest count, grown by a quarter)
    assert U.host_batch_plan(tab["eol"]) is True and U.host_plan(tab["eol"])["contexts"] != 1
    ends_cr = [i for i, d in enumerate(ins["batch"]) if d.endswith(b"\r")]
    assert ends_cr == [child_mod.BATCH_CR] and len(ins["batch"]) == 64
    lens = [len(d) for d in ins["batch"]]
    assert lens == sorted(lens) and lens[0] == 256 and lens[-1] == 8192
    left = max(counts[-1], want["stream"][0])
    assert sum(w[0] for w in want["batch"]) > 2 * (left + left // 4)
    assert sum(1 for w in want["batch"] if w[0]) > 32
    # 4. / 5.
    assert 0 < want["records"][0][0] < want["records"][1][0]
    for d, w in zip(ins["utf8"], want["utf8"]):
        assert w == dict(first_bad=d.size - 5, binary=True, nul=None)


@pytest.fixture(scope="module")
def child():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    r = subprocess.run([sys.executable, os.path.join(HERE, "ws_growth_child.py")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout.decode().strip().split("\n")[-1])


@pytest.mark.gpu
def test_find_all_regrows(child, want):
    assert child["find_all"] == want["find_all"]


@pytest.mark.gpu
def test_stream_carry_survives_regrow(child, want):
    assert child["stream"] == want["stream"]


@pytest.mark.gpu
def test_batch_keep_growth(child, want):
    b = child["batch"]
    assert b["contexts"] != 1 and b["one_scan"] is False
    assert b["count"] == sum(w[0] for w in want["batch"])
    for i, w in enumerate(want["batch"]):
        assert b["got"][i] == w, i
        assert b["find_all"][i] == w, i


@pytest.mark.gpu
def test_records_regrow(child, want):
    assert child["records"] == want["records"]


@pytest.mark.gpu
def test_binary_tests(child, want):
    assert child["utf8"] == want["utf8"]
