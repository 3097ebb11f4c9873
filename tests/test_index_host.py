"""CPU: the model of the file index (tests/index_model.py) against the
reference indexer's recorded records (tests/golden/index_cases.json), the
sizing bound the device call relies on, and the store writer and parser of the
package against the model's and against a store the reference wrote.  The
first guards the model the GPU tests compare with."""
import json
import os

import numpy as np
import pytest

import index_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_cases.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def modelled(golden):
    """Per case: the decoded bytes, the binary flag and the unfolded table, computed once."""
    out = {}
    for case in golden["cases"]:
        data = M.decoded(M.input_of(case["input"]))
        out[case["name"]] = (data, M.is_binary(data) if data else False, M.hash_table(data) if data else None)
    return out


def test_golden_inputs_are_the_models(golden):
    names = [c["name"] for c in golden["cases"]]
    assert names == [n for n, _, _ in M.golden_inputs()]
    assert len([n for n in names if n.startswith("flag_")]) == 14
    for (name, spec, data), case in zip(M.golden_inputs(), golden["cases"]):
        assert case["input"] == spec and M.input_of(spec) == data, name
        assert len(case["rows"]) == 20


def test_model_reproduces_every_recorded_record(golden, modelled):
    checked = 0
    for case in golden["cases"]:
        data, binary, table = modelled[case["name"]]
        for acc, ib, header, tlen, ref, pct in case["rows"]:
            where = (case["name"], acc, ib)
            if not data:
                want = (0, b"", 0)
            elif binary and ib:
                want = (0x80, b"", 0)
            else:
                t, z = M.fold(table, acc)
                want = ((t.size.bit_length() - 1) | (0x80 if binary else 0), t.tobytes(), z)
            assert want[0] == header, where
            assert len(want[1]) == tlen, where
            if tlen:
                assert (tlen <= 4096) == isinstance(ref, int), where
                if tlen <= 4096:
                    assert want[1] == bytes.fromhex(golden["tables"][ref]), where
                else:
                    assert M.table_sha(want[1]) == ref, where
            assert M.noise_percent(want[2], tlen) == pct, where
            checked += 1
    assert checked == 36 * 20


def test_index_record_is_that_composition(golden):
    for case in golden["cases"][:20]:
        data = M.decoded(M.input_of(case["input"]))
        for acc, ib, header, tlen, ref, _ in case["rows"][6:10]:
            h, t, _ = M.index_record(data, acc, bool(ib))
            assert (h, len(t)) == (header, tlen)
            assert not tlen or (t.hex() == golden["tables"][ref] if isinstance(ref, int) else M.table_sha(t) == ref)


def test_recorded_flags_are_what_the_cases_say(golden):
    by = {c["name"]: c for c in golden["cases"]}
    binary = {n: bool(by["flag_" + n]["rows"][8][2] & 0x80) for n, _ in M.crafted_flag_cases()}
    assert binary == {"nul": True, "latin1": True, "c0_lead": True, "f5_lead": True, "surrogate": False,
                      "overlong3": False, "overlong4": False, "lone_cont": True, "tail_lead": False,
                      "tail_conts": True, "nul_before_window": True, "nul_after_window": False,
                      "window_in_2byte": False, "window_in_3byte": False}
    # -I: a binary input has the flag and no table
    for n, b in binary.items():
        row = by["flag_" + n]["rows"][9]
        assert row[1] == 1 and (row[2], row[3]) == ((0x80, 0) if b else (row[2] & 0x7F, 1 << row[2]))


def test_fold_extremes_are_recorded(golden):
    by = {c["name"]: c for c in golden["cases"]}
    assert all(r[3] == 65536 for r in by["gen_random_1048576_11"]["rows"] if not r[1])  # (binary: no table under -I)
    assert all(r[3] == 128 for r in by["gen_words_1_1"]["rows"])
    sizes = {r[3] for r in by["gen_words_4096_6"]["rows"]}
    assert len(sizes) >= 3 and max(sizes) < 65536 and min(sizes) > 128


def test_sizing_bound_holds_and_is_tight_in_kind():
    """A final table never exceeds slot_bound, whatever the bytes: checked on
    inputs that clear the most bits for their length (random bytes)."""
    for n in (1, 2, 5, 31, 32, 33, 100, 1000, 3000, 20000, 52428, 52429, 70000):
        data = M.gen_input("random", n, n)
        table = M.hash_table(data)
        for acc in range(10):
            t, _ = M.fold(table, acc)
            bound = M.slot_bound(n, acc)
            assert t.size <= bound, (n, acc)
            assert bound == 128 or (bound // 2) * M.MAX_NOISE[acc] <= 100 * n < bound * M.MAX_NOISE[acc] or bound == 65536


def test_fold_equals_hashing_modulo_the_size():
    """Folding to `size` bytes equals indexing with h mod size: the device call
    hashes into a table of the sizing bound from the start."""
    data = np.frombuffer(M.gen_input("words", 3000, 1), np.uint8).astype(np.uint32)
    table = M.hash_table(data)
    for size in (32768, 4096, 128):
        folded = table.reshape(-1, size)
        folded = np.bitwise_and.reduce(folded, axis=0)
        direct = np.full(size, 0xFF, np.uint8)
        h = data.copy()
        for k in range(8):
            if k:
                h = (61 * h[:data.size - k] + data[k:]) & 0xFFFF
            np.bitwise_and.at(direct, h & (size - 1), np.uint8(0xFF ^ (1 << k)))
        assert np.array_equal(folded, direct), size


# ---- the package's store writer and parser (host code)

def test_store_writer_and_parser_round_trip():
    import ugrep_amd as U
    recs = []
    for i, (kind, n) in enumerate((("words", 0), ("words", 5), ("random", 900), ("low", 3000), ("repeat", 10))):
        h, t, _ = M.index_record(M.gen_input(kind, n, i), 6)
        recs.append(("file%d.txt" % i if i else "ünï.txt", h, t))
    blob = U.write_index_store([r[0] for r in recs], [(r[1], r[2]) for r in recs], 6)
    assert blob == M.store_bytes(recs, 6)
    parsed = U.parse_index_store(blob)
    assert parsed == M.parse_store(blob)
    assert parsed == [(nm.encode(), 6, h, t) for nm, h, t in recs]
    assert U.write_index_store([p[0] for p in parsed], [(p[2], p[3]) for p in parsed], 6) == blob
    assert U.parse_index_store(U.write_index_store([], [], 0)) == []


def test_store_writer_and_parser_reject_bad_input():
    import ugrep_amd as U
    with pytest.raises(ValueError):
        U.write_index_store(["a"], [(7, b"")], 4)          # a header that promises 128 bytes
    with pytest.raises(ValueError):
        U.write_index_store(["a"], [(0, b"")], 10)
    with pytest.raises(ValueError):
        U.write_index_store(["a", "b"], [(0, b"")], 4)
    with pytest.raises(ValueError):
        U.parse_index_store(b"UG#\x02\x00")
    good = U.write_index_store(["a"], [(7, b"\xff" * 128)], 4)
    with pytest.raises(ValueError):
        U.parse_index_store(good[:-1])


def test_store_of_a_one_file_directory_equals_the_reference(golden):
    import ugrep_amd as U
    one = golden["one_file_store"]
    h, t, _ = M.index_record(bytes.fromhex(one["input_hex"]), one["accuracy"])
    assert U.write_index_store([one["name"]], [(h, t)], one["accuracy"]).hex() == one["store_hex"]
    (name, acc, header, table), = U.parse_index_store(bytes.fromhex(one["store_hex"]))
    assert (name.decode(), acc, header, table) == (one["name"], one["accuracy"], h, t)


def test_argument_checks_come_before_the_device():
    import ctypes

    import ugrep_amd as U
    from ugrep_amd import _lib
    with pytest.raises(_lib.UgpuError) as ei:
        U.index_batch([b"abc"], accuracy=10)
    assert ei.value.code == _lib.UGPU_INVAL
    with pytest.raises(_lib.UgpuError) as ei:
        U.index_tables(0, 0, [0, 0], accuracy=12)
    assert ei.value.code == _lib.UGPU_INVAL
    with pytest.raises(_lib.UgpuError) as ei:
        U.index_tables(16, 8, [0, 5, 3])
    assert ei.value.code == _lib.UGPU_INVAL
    with pytest.raises(_lib.UgpuError) as ei:
        U.index_tables(16, 8, [0, 9])
    assert ei.value.code == _lib.UGPU_INVAL
    res = U.index_batch([])
    assert len(res) == 0 and res.tables.size == 0 and list(res.offset) == [0]
    assert _lib.lib.ugpu_abi_version() == 3
    assert isinstance(U.index_chunk(), int) and U.index_chunk() % 4096 == 0
    del ctypes
