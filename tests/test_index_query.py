"""GPU: ugpu_index_query / ugpu_index_query_store (the index query kernel of
index_query.hip) against the reference CLI's recorded decisions
(tests/golden/hfa_cases.json), the host evaluator ugpu_hfa_match_host and the
Python restatement tests/hfa_model.py, which tests/test_hfa_host.py ties to
each other on the CPU.  Every comparison is exact."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import hfa_model as H
import index_model as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF_UGREP = os.path.join(REPO, "oracle", "_ref", "ugrep")
ACCURACIES = (0, 4, 9)


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "hfa_cases.json")) as f:
        g = json.load(f)
    assert g["corpus"] == H.corpus() and g["patterns"] == H.patterns()
    g["files"] = [(c["name"], H.corpus_bytes(c)) for c in g["corpus"]]
    with open(os.path.join(HERE, "golden", "hfa_diverge.json")) as f:
        g["diverge"] = json.load(f)["patterns"]
    return g


def query_of(U, p):
    return U.IndexQuery(p["pattern"], fixed="-F" in p["args"], icase="-i" in p["args"])


@pytest.fixture(scope="module")
def pool():
    """Records of every table size, as (header, table): the shared inputs of the tests below."""
    datas = [M.gen_input("words", n, 40 + i) for i, n in enumerate((1, 9, 100, 800, 3000, 12000, 50000, 200000))]
    datas += [M.gen_input("utf8", 4000, 5), M.gen_input("ascii", 2000, 6), b"a" * 777,
              b"needle07 kernel " * 3, M.gen_input("random", 30000, 7)]
    recs = [M.index_record(d, acc)[:2] for d in datas for acc in (2, 9)]
    recs += [M.index_record(M.gen_input("words", 1500, 1) + b"the kernel of it\n", acc)[:2] for acc in (0, 7)]
    recs += [(0, b""), (0x80, b"")]
    assert {len(t) for _, t in recs} >= {0, 128, 256, 1024, 4096, 8192, 65536}
    return recs


def as_store(recs):
    return [(b"r%d" % i, 4, h, t) for i, (h, t) in enumerate(recs)]


def host_keep(q, recs, **kw):
    return np.array([q.keep_host(h, t, **kw) for h, t in recs], bool)


def test_every_recorded_triple(U, golden):
    names = [nm for nm, _ in golden["files"]]
    results = {acc: U.index_batch([d for _, d in golden["files"]], accuracy=acc) for acc in ACCURACIES}
    for acc in ACCURACIES:   # (the tables are the model's, which made the fixture's stores)
        for i, (_, d) in enumerate(golden["files"]):
            h, t, _ = M.index_record(d, acc)
            assert (int(results[acc].header[i]), results[acc].table(i)) == (h, t)
    queries = [query_of(U, p) for p in golden["patterns"]]
    for r in golden["rows"]:
        p, acc = golden["patterns"][r["pattern"]], r["accuracy"]
        q = queries[r["pattern"]]
        res = results[acc]
        keep = q.query(res)
        host = host_keep(q, [(int(res.header[i]), res.table(i)) for i in range(len(res))])
        assert np.array_equal(keep, host), (p, acc)
        if p["pattern"] not in golden["diverge"]:
            assert sorted(nm for nm, k in zip(names, keep) if k) == sorted(r["kept"]), (p, acc)


def test_table_sizes_and_header_rules(U):
    q = U.IndexQuery("kernel")
    text = b"the kernel of it\n"
    rnd = M.gen_input("random", 1 << 20, 11)
    small = M.index_record(text, 4)
    mid = M.index_record(M.gen_input("words", 300, 1) + text, 2)
    big = M.index_record(rnd, 9)
    none = M.index_record(M.gen_input("words", 300, 1), 4)
    assert (len(small[1]), len(mid[1]), len(big[1]), big[0]) == (128, 256, 65536, 0x90)
    recs = [small[:2], mid[:2], big[:2], none[:2], (0, b""), (0x80, b""), (0x80 | small[0], small[1]),
            (0x20 | small[0], small[1]), (0x40 | small[0], small[1]), (0x20, b""), (0xC0, b"")]
    none_q = U.IndexQuery("a*")
    res = U.index_batch([text, rnd[:5000], b""])
    for kw in ({}, {"ignore_binary": True}, {"decompress": True}, {"ignore_binary": True, "decompress": True}):
        for qq in (q, none_q):   # (without an automaton the header rules do not apply: every record is kept)
            got = qq.query(as_store(recs), **kw)
            want = np.array([H.keep_record(qq.words(), h, t, **kw) for h, t in recs], bool)
            assert np.array_equal(got, want), kw
            assert np.array_equal(got, host_keep(qq, recs, **kw)), kw
            assert np.array_equal(got, qq.query(as_store(recs), device=False, **kw)), kw
            assert np.array_equal(qq.query(res, **kw), qq.query(res, device=False, **kw)), kw
        assert none_q.query(as_store(recs), **kw).all()
    assert U.IndexQuery.kernel_ms() >= 0
    plain = q.query(as_store(recs))
    assert list(plain[:7]) == [True, True, q.match_host(big[1]), False, False, True, True]
    assert not plain[7] and not plain[8] and not plain[9] and not plain[10]
    assert list(q.query(as_store(recs), ignore_binary=True)[4:7]) == [False, False, False]
    assert list(q.query(as_store(recs), decompress=True)[7:]) == [True, True, False, True]
    assert U.IndexQuery("a*").query(as_store(recs)).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000])
def test_record_counts_and_permutation(U, pool, n):
    rs = np.random.RandomState(n)
    pick = rs.randint(0, len(pool), n)
    recs = [pool[i] for i in pick]
    for pat in ("kernel", "[a-z]+que"):
        q = U.IndexQuery(pat)
        by_pool = host_keep(q, pool)
        keep = q.query(as_store(recs))
        assert np.array_equal(keep, by_pool[pick]), pat
        perm = rs.permutation(n)
        assert np.array_equal(q.query(as_store([recs[i] for i in perm])), keep[perm]), pat
    if n == 3000:
        assert 0 < int(keep.sum()) < n


def test_wide_levels_and_wide_ranges(U, pool):
    words = U.IndexQuery("|".join(H.word_set()))
    f = H.Flat(words.words())
    assert max(int(f.level_first[i + 1] - f.level_first[i]) for i in range(16)) > 64
    keep = words.query(as_store(pool))
    assert np.array_equal(keep, host_keep(words, pool)) and 0 < int(keep.sum()) < len(pool)
    wide = U.IndexQuery("\\w+")
    small = [r for r in pool if len(r[1]) == 128]
    assert small and int((H.Flat(wide.words()).hi - H.Flat(wide.words()).lo).max()) >= 128
    assert np.array_equal(wide.query(as_store(small)), host_keep(wide, small))
    for pat in ("[^a-z ]{2}", "[a-z]{3}ord"):
        q = U.IndexQuery(pat)
        assert np.array_equal(q.query(as_store(pool)), host_keep(q, pool)), pat


def test_both_sides_of_the_lds_switch(U, pool):
    assert 128 <= U.lib.ugpu_index_query_lds() <= 65536
    for pat in ("kernel", "[a-z]+que", "\\w+", "|".join(H.word_set())):
        q = U.IndexQuery(pat)
        want = host_keep(q, pool)
        for force in ("lds", "global", None):
            assert np.array_equal(q.query(as_store(pool), force=force), want), (pat, force)


def test_store_blob_equals_the_device_form(U, golden):
    datas = [d for _, d in golden["files"]]
    names = [nm for nm, _ in golden["files"]]
    res = U.index_batch(datas, accuracy=4)
    blob = U.write_index_store(names, res)
    host = b"".join(datas)
    bounds = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.uint64)
    buf = torch.zeros(len(host) + 32, dtype=torch.uint8, device="cuda")
    buf[:len(host)] = torch.from_numpy(np.frombuffer(host, np.uint8).copy())
    torch.cuda.synchronize()
    header, _, offset, total = U.index_tables(buf.data_ptr(), len(host), bounds)
    dst = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    header, _, offset, total = U.index_tables(buf.data_ptr(), len(host), bounds, d_tables=dst.data_ptr(), capacity=total)
    for pat in ("kernel", "needle0[1-3]", "zyzzyva", "\\w+"):
        got_names, keep = U.query_index_store(blob, pat)
        assert [n.decode() for n in got_names] == names
        dev = U.IndexQuery(pat).query((dst.data_ptr(), header, offset))
        assert np.array_equal(keep, dev), pat
        assert np.array_equal(keep, U.IndexQuery(pat).query(U.parse_index_store(blob))), pat
    with pytest.raises(U.UgpuError):
        U.query_index_store(blob[:-7], "kernel")


def test_find_indexed_equals_find_batch(U, golden):
    datas = [d for _, d in golden["files"]]
    index = U.index_batch(datas)
    for pat in ("needle17", "kernel|zq1[0-9]x", "[a-z]+que"):
        got = U.find_indexed(pat, datas, index=index)
        want = U.find_batch(U.Pattern(U.compile_regex(pat)), datas)
        assert not got.kept.all() and got.kept.any(), pat
        assert got.count == want.count and want.count > 0
        for a in ("first", "digest", "dcap", "newlines", "matching_lines", "start", "length", "cap", "line"):
            assert np.array_equal(getattr(got, a), getattr(want, a)), (pat, a)
    got = U.find_indexed("a*", datas)          # no automaton: indexed here, every input scanned
    want = U.find_batch(U.Pattern(U.compile_regex("a*")), datas)
    assert got.kept.all() and got.count == want.count and np.array_equal(got.start, want.start)


def test_reference_cli_keeps_the_same_files(U, tmp_path):
    if not os.path.exists(REF_UGREP):
        pytest.skip("oracle/_ref/ugrep is not built")
    d = tmp_path / "verify"
    shutil.copytree(os.path.join(HERE, "golden", "verify"), d)
    for e in os.scandir(d):   # ugrep searches a file whose time stamp is later than the store's
        os.utime(e.path, (e.stat().st_atime - 100, e.stat().st_mtime - 100))
    names, _ = U.index_directory(str(d))
    skipped = 0
    for pat in ("Hello", "dolor|World", "zyzzyvaword"):
        r = subprocess.run([REF_UGREP, "--index=log", "-rl", "-e", pat, "."], cwd=d, stdin=subprocess.DEVNULL,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode in (0, 1), r.stderr
        log = r.stderr.decode()
        assert "(changed)" not in log and "(not indexed)" not in log, log
        ref = sorted(os.path.normpath(ln[len("INDEX LOG: "):].split(" (")[0]) for ln in log.splitlines()
                     if ln.startswith("INDEX LOG: "))
        got_names, keep = U.query_index_store(str(d / "._UG#_Store"), pat)
        assert sorted(n.decode() for n, k in zip(got_names, keep) if k) == ref, pat
        skipped += len(names) - len(ref)
    assert skipped > 0
