"""bench.py's plain run, --full and --dump-outputs.

CPU: dump_outputs() writes the last step's result as float64 .npy files, the
u64 sums as exact 32-bit halves, and of a long record list a fixed sample.
GPU: a plain run on a small buffer times exactly --steps steps, runs none of
the --full legs and dumps the totals of its result line; --full adds the legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_KEYS = ("cpu_baseline", "pcie_inclusive", "parity_vs_reference")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _u64(halves):
    return (int(halves[0]) << 32) | int(halves[1])


def test_dump_totals_exact(tmp_path):
    import bench
    res = dict(count=3, digest=0xFEDCBA9876543211, dcap=(1 << 64) - 1, exit=(1 << 34) + 5, entry=0)
    bench.dump_outputs(str(tmp_path / "o"), res)
    got = _load(str(tmp_path / "o"))
    assert sorted(got) == ["count", "dcap", "digest", "exit"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["count"].tolist() == [3.0] and got["exit"].tolist() == [float((1 << 34) + 5)]
    assert _u64(got["digest"]) == res["digest"] and _u64(got["dcap"]) == res["dcap"]


def test_dump_records_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    # two per-rank parts, as a gather to rank 0 returns them; 12-byte records (no accept)
    st = [torch.arange(0, 700, dtype=torch.int64) * 3, torch.arange(0, 500, dtype=torch.int64) * 3 + (1 << 33)]
    ln = [torch.full((700,), 2, dtype=torch.int32), torch.full((500,), 5, dtype=torch.int32)]
    res = dict(count=1200, digest=1, dcap=0, exit=9, records=(st, ln, [None, None], "gather"))
    bench.dump_outputs(str(tmp_path / "all"), res)
    got = _load(str(tmp_path / "all"))
    assert "records_accept" not in got and "records_index" not in got
    assert np.array_equal(got["records_start"], torch.cat(st).numpy().astype(np.float64))
    assert np.array_equal(got["records_len"], torch.cat(ln).numpy().astype(np.float64))

    monkeypatch.setattr(bench, "DUMP_RECORDS", 100)
    ac = [torch.arange(700, dtype=torch.int32) % 3, torch.arange(500, dtype=torch.int32) % 3]
    res["records"] = (st, ln, ac, "gather")
    bench.dump_outputs(str(tmp_path / "s1"), res)
    bench.dump_outputs(str(tmp_path / "s2"), res)
    s1, s2 = _load(str(tmp_path / "s1")), _load(str(tmp_path / "s2"))
    assert sorted(s1) == sorted(s2) and all(np.array_equal(s1[k], s2[k]) for k in s1)  # the same sample every time
    idx = s1["records_index"].astype(np.int64)
    assert idx.size == 100 and np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < 1200
    assert idx.max() >= 700  # (both parts are drawn from)
    assert np.array_equal(s1["records_start"], torch.cat(st).numpy()[idx].astype(np.float64))
    assert np.array_equal(s1["records_len"], torch.cat(ln).numpy()[idx].astype(np.float64))
    assert np.array_equal(s1["records_accept"], torch.cat(ac).numpy()[idx].astype(np.float64))
    assert all(a.dtype == np.float64 for a in s1.values())


def _bench(args):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--bytes", str(8 << 20)] + args,
                         capture_output=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout.decode()
    return json.loads(lines[0]), out.stderr.decode()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_result(tmp_path):
    d = str(tmp_path / "dump")
    j, err = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", d])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0
    assert j["unit"] == "GB/s" and j["higher_is_better"] is True and j["dtype"] == "u8"
    # value is the steps' own rate: bytes x steps / their time
    assert j["value"] == pytest.approx((8 << 20) / (j["ms_per_step"] * 1e-3) / 1e9, rel=0.02, abs=0.006)
    assert not any(k in j for k in FULL_KEYS), sorted(j)
    assert "cpu baseline" not in err
    got = _load(d)
    assert sorted(got) == ["count", "dcap", "digest", "exit"]
    assert got["count"].tolist() == [float(j["matches"])] and j["matches"] > 0
    assert _u64(got["digest"]) == j["digest"]
    assert 0 < got["exit"][0] <= float(8 << 20)


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
    j, _ = _bench(["--steps", "2", "--warmup", "1", "--full"])
    assert j["steps"] == 2
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["kind"] in ("reference", "port")
    assert j["pcie_inclusive"]["equals_device_resident"] is True
    if j["cpu_baseline"]["kind"] == "reference":
        assert j["parity_vs_reference"]["equal"] is True
