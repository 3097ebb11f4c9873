"""GPU: ugpu_index_batch / ugpu_index_tables (ugrep-indexer's hash tables, their
folding and the binary flag) against the model of tests/index_model.py and the
reference indexer's recorded records (tests/golden/index_cases.json), which
tests/test_index_host.py ties to each other.  Every comparison is exact: the
header byte, the table's bytes and its zero-bit count."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import index_model as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF_UGREP = os.path.join(REPO, "oracle", "_ref", "ugrep")


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import ugrep_amd
    return ugrep_amd


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "index_cases.json")) as f:
        g = json.load(f)
    for c in g["cases"]:
        c["tables"] = g["tables"]
    g["by"] = {c["name"]: c for c in g["cases"]}
    return g


@pytest.fixture(scope="module")
def text(U):
    """One text of 3 chunks and an odd tail; the tests below take slices of it."""
    return M.gen_input("words", 3 * U.index_chunk() + 12345, 21)


def check_model(res, inputs, accuracy=4, ignore_binary=False):
    assert len(res) == len(inputs)
    for i, data in enumerate(inputs):
        h, t, z = M.index_record(data, accuracy, ignore_binary)
        assert int(res.header[i]) == h, (i, len(data))
        assert int(res.zero_bits[i]) == z, (i, len(data))
        assert res.table(i) == t, (i, len(data))


def check_golden(res, i, case, accuracy, ignore_binary):
    (row,) = [r for r in case["rows"] if r[0] == accuracy and r[1] == int(ignore_binary)]
    _, _, header, tlen, ref, pct = row  # ref: the table's place in "tables" up to 4096 bytes, its SHA-256 beyond
    where = (case["name"], accuracy, ignore_binary)
    assert int(res.header[i]) == header, where
    assert len(res.table(i)) == tlen, where
    if tlen:
        assert res.table(i).hex() == case["tables"][ref] if isinstance(ref, int) else M.table_sha(res.table(i)) == ref, where
    assert res.noise_percent(i) == pct, where


def test_lengths_around_the_window_and_the_chunk(U, text):
    C = U.index_chunk()
    lens = [0, 1, 2, 7, 8, 9, 15, 16, 17] + list(range(C - 8, C + 9)) + list(range(2 * C - 8, 2 * C + 9))
    inputs = [text[:n] for n in lens]
    check_model(U.index_batch(inputs), inputs)


def test_wrapping_hashes(U, golden):
    C = U.index_chunk()
    inputs = [b"\xff" * 70000, b"a" * 777, b"\xff" * 9, b"\xff" * (C + 100), b"\x00" * 5000, b"z" * (2 * C + 3)]
    for acc in (4, 9):
        res = U.index_batch(inputs, accuracy=acc)
        check_model(res, inputs, acc)
        check_golden(res, 0, golden["by"]["gen_repeat_70000_255"], acc, False)
        check_golden(res, 1, golden["by"]["gen_repeat_777_97"], acc, False)


def test_an_8gram_across_a_chunk_boundary_is_indexed(U):
    """The gram's bytes occur nowhere else, and the background is one repeated
    byte, so the table folds to 128 bytes and few of its bits are cleared: the
    bits of the gram's eight prefixes are cleared with it and not all without."""
    C = U.index_chunk()
    gram = bytes(range(1, 9))
    hs, h = [], 0
    for k, b in enumerate(gram):
        h = (61 * h + b) & 0xFFFF if k else b
        hs.append(h)
    plain = b"a" * (2 * C)
    inputs = [plain] + [plain[:C - s] + gram + plain[C - s + 8:] for s in range(1, 8)]
    res = U.index_batch(inputs, accuracy=9)
    check_model(res, inputs, 9)

    def cleared(i):
        t = np.frombuffer(res.table(i), np.uint8)
        return [not (int(t[h & (t.size - 1)]) >> k) & 1 for k, h in enumerate(hs)]
    assert not all(cleared(0))
    for i in range(1, 8):
        assert len(inputs[i]) == 2 * C and all(cleared(i)), i


def test_many_small_inputs_do_not_see_their_neighbours(U):
    rs = np.random.RandomState(5)
    alphabet = np.frombuffer(b"abcdefgh \n\xc3\xa9\xe2\x82\xac\xf0", np.uint8)
    lens = rs.randint(0, 41, 300)
    lens[[0, 1, 2, 50, 51, 52, 53, 120, 200, 201, 298, 299]] = 0
    inputs = [alphabet[rs.randint(0, alphabet.size, n)].tobytes() for n in lens]
    for ib in (False, True):
        res = U.index_batch(inputs, ignore_binary=ib)
        check_model(res, inputs, 4, ib)
        assert {bool(h & 0x80) for h in res.header} == {False, True}
        for i in range(0, 300, 7):
            alone = U.index_batch([inputs[i]], ignore_binary=ib)
            assert (int(alone.header[0]), int(alone.zero_bits[0]), alone.table(0)) == \
                (int(res.header[i]), int(res.zero_bits[i]), res.table(i)), i


def test_fold_extremes(U, golden):
    never, small, between = "gen_random_1048576_11", "gen_words_1_1", "gen_words_4096_6"
    inputs = [M.input_of(golden["by"][n]["input"]) for n in (never, small, between)]
    sizes = set()
    for acc in range(10):
        res = U.index_batch(inputs, accuracy=acc)
        for i, n in enumerate((never, small, between)):
            check_golden(res, i, golden["by"][n], acc, False)
        assert len(res.table(0)) == 65536 and len(res.table(1)) == 128 and 128 < len(res.table(2)) < 65536
        sizes.add(len(res.table(2)))
        if acc in (0, 4, 9):
            check_model(res, inputs, acc)
    assert len(sizes) >= 4


@pytest.mark.parametrize("ignore_binary", [False, True])
def test_binary_flag_cases(U, golden, ignore_binary):
    cases = M.crafted_flag_cases()
    assert len(cases) == 14
    inputs = [d for _, d in cases]
    res = U.index_batch(inputs, ignore_binary=ignore_binary)
    check_model(res, inputs, 4, ignore_binary)
    for i, (name, _) in enumerate(cases):
        check_golden(res, i, golden["by"]["flag_" + name], 4, ignore_binary)


def test_every_recorded_case(U, golden):
    plain = [c for c in golden["cases"] if not c["name"].startswith("bom_")]
    inputs = [M.input_of(c["input"]) for c in plain]
    for acc, ib in ((4, False), (7, True), (0, False)):
        res = U.index_batch(inputs, accuracy=acc, ignore_binary=ib)
        for i, c in enumerate(plain):
            check_golden(res, i, c, acc, ib)


def test_encodings_with_a_bom(U, golden):
    cases = [c for c in golden["cases"] if c["name"].startswith("bom_")]
    assert len(cases) == 6
    raws = [M.input_of(c["input"]) for c in cases]
    for ib in (False, True):
        res = U.index_inputs(raws, ignore_binary=ib)
        check_model(res, [M.decoded(r) for r in raws], 4, ib)
        for i, c in enumerate(cases):
            check_golden(res, i, c, 4, ib)
    # the same bytes taken as they are give other records
    assert U.index_batch(raws).table(2) != U.index_inputs(raws).table(2)


def test_three_chunks_and_a_tail_beside_small_inputs(U, text, golden):
    big = M.input_of(golden["by"]["gen_words_800001_12"]["input"])
    assert len(big) > 3 * U.index_chunk() and len(big) % U.index_chunk()
    inputs = [text[:100], text, b"", text[5:3000], big, b"\x00binary" + text[:2 * U.index_chunk() + 1], text[:17]]
    for acc, ib in ((4, False), (7, True)):
        res = U.index_batch(inputs, accuracy=acc, ignore_binary=ib)
        check_model(res, inputs, acc, ib)
        check_golden(res, 4, golden["by"]["gen_words_800001_12"], acc, ib)


def test_sub_batches_and_workspace_groups_give_the_same(U, text, monkeypatch):
    C = U.index_chunk()
    inputs = [text[i * 997:i * 997 + n] for i, n in enumerate([0, 3000, C + 5, 40, 0, 70000, 2 * C + 9, 1, 20000, 0])]
    want = U.index_batch(inputs, accuracy=6)
    check_model(want, inputs, 6)
    for name, value in (("UGPU_BATCH_BYTES", "65536"), ("UGPU_INDEX_WS_BYTES", "1")):
        monkeypatch.setenv(name, value)
        got = U.index_batch(inputs, accuracy=6)
        monkeypatch.delenv(name)
        assert np.array_equal(got.header, want.header) and np.array_equal(got.zero_bits, want.zero_bits)
        assert np.array_equal(got.offset, want.offset) and np.array_equal(got.tables, want.tables)


def test_device_entry_segments_capacity_and_size_query(U, text):
    """ugpu_index_tables over segments of one buffer, empty ones among them:
    every other segment is 00 E2 82, which would change its neighbours' flags
    and tables if a window or the flag's look-back crossed a bound."""
    C = U.index_chunk()
    segs = []
    for part in (text[:50], b"", text[50:50 + C + 3], b"caf\xc3\xa9", text[7:9], b"\x82\xac ok"):
        segs += [part, b"\x00\xe2\x82"]
    host = b"".join(segs)
    bounds = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    buf = torch.zeros(len(host) + 16, dtype=torch.uint8, device="cuda")
    buf[:len(host)] = torch.from_numpy(np.frombuffer(host, np.uint8).copy())
    torch.cuda.synchronize()
    header, zeros, offset, total = U.index_tables(buf.data_ptr(), len(host), bounds)
    assert total == sum(len(M.index_record(s)[1]) for s in segs) and int(offset[-1]) == total
    dst = torch.full((total + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h2, z2, o2, t2 = U.index_tables(buf.data_ptr(), len(host), bounds, d_tables=dst.data_ptr(), capacity=total)
    out = dst.cpu().numpy()
    assert t2 == total and np.array_equal(h2, header) and np.array_equal(z2, zeros) and np.array_equal(o2, offset)
    assert np.all(out[total:] == 0xA5), "bytes written behind tables_len"
    for i, s in enumerate(segs):
        h, t, z = M.index_record(s)
        assert (int(header[i]), int(zeros[i])) == (h, z), i
        assert out[int(offset[i]):int(offset[i + 1])].tobytes() == t, i
    with pytest.raises(U.UgpuError) as ei:
        U.index_tables(buf.data_ptr(), len(host), bounds, d_tables=dst.data_ptr(), capacity=total - 128)
    assert ei.value.code == 6 and ei.value.out_len == total
    assert U.index_tables(buf.data_ptr(), len(host), [0])[3] == 0


def test_index_directory_serves_the_reference_cli(U, tmp_path):
    if not os.path.exists(REF_UGREP):
        pytest.skip("oracle/_ref/ugrep is not built")
    d = tmp_path / "verify"
    shutil.copytree(os.path.join(HERE, "golden", "verify"), d)
    # ugrep searches a file whose time stamp is later than the store's whatever the store says
    for e in os.scandir(d):
        os.utime(e.path, (e.stat().st_atime - 100, e.stat().st_mtime - 100))
    names, res = U.index_directory(str(d))
    assert names == sorted(os.listdir(os.path.join(HERE, "golden", "verify")))
    with open(d / "._UG#_Store", "rb") as f:
        parsed = U.parse_index_store(f.read())
    assert [p[0].decode() for p in parsed] == names
    for nm, (_, acc, header, table) in zip(names, parsed):
        with open(d / nm, "rb") as f:
            h, t, _ = M.index_record(M.decoded(f.read()))
        assert (acc, header, table) == (4, h, t), nm

    def files(args):
        r = subprocess.run([REF_UGREP] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode in (0, 1), r.stderr
        return sorted(r.stdout.decode().split()), r.stderr.decode()
    skipped = 0
    for pat in ("Hello", "Lorem ipsum", "dolor|World", "[a-z]+que", "main\\(", "zyzzyvaword"):
        want, _ = files(["-rl", pat])
        got, log = files(["--index=log", "-rl", pat])
        assert got == want, pat
        assert "(changed)" not in log and "(not indexed)" not in log, log
        skipped += len(names) - log.count("INDEX LOG:")
    assert skipped > 0, "the store never let the CLI skip a file"
