"""The file index of ugrep-indexer restated in numpy: the hash table of 1- to
8-grams, its folding by the noise rule, the binary flag, the record and the
store format, and the seeded inputs the fixtures and the GPU tests share.

The table: 65536 bytes of 0xff; for every position i and k in 0..7 with
i + k < n, bit k of table[h(i, k)] is cleared, h(i, 0) = byte[i] and
h(i, k) = (61 * h(i, k-1) + byte[i+k]) mod 2^16.  The fold: while size > 128,
AND the halves and count the zero bits z of the result; stop when
100 * z >= max_noise * 8 * half, otherwise keep the result.  tests/golden/
index_cases.json (make_index_golden.py) ties all of it to the reference
indexer."""
import hashlib

import numpy as np

MAX_NOISE = (80, 73, 65, 57, 49, 42, 34, 26, 18, 10)  # by accuracy 0..9
TABLE = 65536
MIN_TABLE = 128
WINDOW = 65536  # the bytes the binary flag looks at
MAGIC = b"UG#\x03\x00"
STORE_NAME = "._UG#_Store"


def as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def hash_table(data):
    """The unfolded table of the bytes."""
    b = as_u8(data).astype(np.uint32)
    n = b.size
    table = np.full(TABLE, 0xFF, dtype=np.uint8)
    h = b.copy()
    for k in range(min(8, n)):
        if k:
            h = (61 * h[:n - k] + b[k:]) & 0xFFFF
        hit = np.zeros(TABLE, dtype=bool)
        hit[h] = True
        table[hit] &= np.uint8(0xFF ^ (1 << k))
    return table


def zero_bits(table):
    return int(table.size * 8 - np.unpackbits(table).sum())


def fold(table, accuracy):
    """The noise rule applied in order from 65536 down: (table, zero bits)."""
    mx = MAX_NOISE[accuracy]
    z = zero_bits(table)
    while table.size > MIN_TABLE:
        half = table.size // 2
        t = table[:half] & table[half:]
        zh = zero_bits(t)
        if 100 * zh >= mx * 8 * half:
            break
        table, z = t, zh
    return table, z


def is_binary(data):
    """The indexer's flag over the first WINDOW bytes: a trailing sequence is
    cut first (and never checked), then a NUL, a lead byte outside C2..F4, or
    a lead without its continuation bytes makes the input binary.  Surrogates
    and 3/4-byte overlongs pass."""
    w = as_u8(data)[:WINDOW]
    end = w.size
    binary = False
    if end and w[end - 1] & 0x80:
        k = min(end, 4)
        while k > 0:
            end -= 1
            if (w[end] & 0xC0) != 0x80:
                break
            k -= 1
        if (w[end] & 0xC0) != 0xC0:
            binary = True
    if binary:
        return True
    w = w[:end]
    stops = np.flatnonzero((w == 0) | (w >= 0x80))  # only these bytes need a look
    s = 0
    for p in stops.tolist():
        if p < s:  # a continuation byte already consumed
            continue
        c = int(w[p])
        if c < 0xC2 or c > 0xF4:
            return True
        need = 1 + (c >= 0xE0) + (c >= 0xF0)
        for q in range(p + 1, p + 1 + need):
            if q >= end or (int(w[q]) & 0xC0) != 0x80:
                return True
        s = p + 1 + need
    return False


def noise_percent(zeros, size):
    """What ugrep-indexer -v prints for a file."""
    return int(100.0 * zeros / (8 * size) + 0.5) if size else 0


def index_record(data, accuracy=4, ignore_binary=False):
    """(header byte, table bytes, zero bits) of one input's record."""
    b = as_u8(data)
    if not b.size:
        return 0, b"", 0
    binary = is_binary(b)
    if binary and ignore_binary:
        return 0x80, b"", 0
    table, z = fold(hash_table(b), accuracy)
    return (table.size.bit_length() - 1) | (0x80 if binary else 0), table.tobytes(), z


def slot_bound(n, accuracy):
    """The largest final table of an n-byte input: a half of `half` bytes with
    half * max_noise > 100 * n is folded for certain (at most 8n zero bits)."""
    if not n:
        return 0
    size = TABLE
    while size > MIN_TABLE and (size // 2) * MAX_NOISE[accuracy] > 100 * n:
        size //= 2
    return size


def record_bytes(name, accuracy, header, table):
    name = name if isinstance(name, bytes) else name.encode()
    name = name[:65535]
    assert len(table) == ((1 << (header & 0x1F)) if header & 0x1F else 0)
    return bytes([accuracy + 0x30, header, len(name) & 0xFF, len(name) >> 8]) + name + bytes(table)


def store_bytes(records, accuracy):
    """records: (name, header, table) in the order they are written."""
    return MAGIC + b"".join(record_bytes(nm, accuracy, h, t) for nm, h, t in records)


def parse_store(blob):
    """[(name bytes, accuracy, header, table bytes)]"""
    assert blob[:5] == MAGIC, blob[:5]
    out, p = [], 5
    while p < len(blob):
        acc, header, l0, l1 = blob[p:p + 4]
        ln = l0 | (l1 << 8)
        size = (1 << (header & 0x1F)) if header & 0x1F else 0
        name = blob[p + 4:p + 4 + ln]
        table = blob[p + 4 + ln:p + 4 + ln + size]
        assert len(name) == ln and len(table) == size
        out.append((name, acc - 0x30, header, table))
        p += 4 + ln + size
    return out


def table_sha(table):
    return hashlib.sha256(bytes(table)).hexdigest()


# ---- inputs

WORDS = ("the of and to in is that for it as was with be by on not he this are or his from at which but have an had "
         "they you were their one all we can her has there been if more when will would who so no index table hash "
         "file bloom gram noise fold record store binary kernel").split()


def gen_input(kind, n, seed=0):
    """n seeded bytes: 'random' (uniform bytes), 'ascii' (uniform printable),
    'words' (English-like text), 'low' (four letters: few distinct n-grams),
    'repeat' (the byte `seed`), 'utf8' (2- and 3-byte sequences in text)."""
    rs = np.random.RandomState(seed)
    if kind == "random":
        return rs.randint(0, 256, n).astype(np.uint8).tobytes()
    if kind == "ascii":
        return rs.randint(0x20, 0x7F, n).astype(np.uint8).tobytes()
    if kind == "low":
        return np.frombuffer(b"acgt", dtype=np.uint8)[rs.randint(0, 4, n)].tobytes()
    if kind == "repeat":
        return bytes([seed & 0xFF]) * n
    if kind == "words":
        out, size = [], 0
        idx = rs.randint(0, len(WORDS), n // 2 + 2)
        brk = rs.randint(0, 12, n // 2 + 2)
        for i in range(idx.size):
            w = WORDS[idx[i]] + ("\n" if brk[i] == 0 else " ")
            out.append(w)
            size += len(w)
            if size >= n:
                break
        return "".join(out).encode()[:n]
    if kind == "utf8":
        cps = rs.choice(np.array([0x61, 0x20, 0x65, 0xE9, 0x3B1, 0x20AC, 0x4E2D, 0x0A]), n)
        return "".join(map(chr, cps)).encode()[:n]
    raise ValueError(kind)


def bench_pool():
    """16 MiB of text, the bytes tools/bench_index.py and the golden maker's timing use."""
    return b"".join(gen_input("words", 1 << 20, 100 + i) for i in range(16))


def bench_input(pool, i, size):
    """Input i of a bench shape: `size` bytes of the pool, cyclically from an offset that depends on i."""
    start = (i * 7919 * 64) % len(pool)
    return (pool[start:] + pool * (size // len(pool) + 1))[:size]


def crafted_flag_cases():
    """The 14 inputs that pin the binary flag, as (name, bytes)."""
    text = b"a" * (WINDOW + 64)  # (one repeated byte: every table folds to 128 bytes)
    cases = [
        ("nul", b"abc\x00def"),
        ("latin1", b"caf\xe9 au lait\n"),                  # E9 followed by a non-continuation
        ("c0_lead", b"abc\xc0\x80def\n"),                    # 2-byte overlong lead: binary
        ("f5_lead", b"abc\xf5\x80\x80\x80def\n"),            # lead past F4: binary
        ("surrogate", b"abc\xed\xa0\x80def\n"),              # passes
        ("overlong3", b"abc\xe0\x80\x80def\n"),              # passes
        ("overlong4", b"abc\xf0\x80\x80\x80def\n"),          # passes
        ("lone_cont", b"abc\x80def\n"),                      # binary
        ("tail_lead", b"abc\xe2\x82"),                       # incomplete at the end: cut, passes
        ("tail_conts", b"ab\x80\x80\x80\x80"),               # four continuation bytes at the end: binary
        ("nul_before_window", text[:WINDOW - 1] + b"\x00" + text[WINDOW:]),
        ("nul_after_window", text[:WINDOW] + b"\x00" + text[WINDOW + 1:]),
        ("window_in_2byte", text[:WINDOW - 1] + "é".encode() + text[WINDOW + 1:]),
        ("window_in_3byte", text[:WINDOW - 2] + "€".encode() + text[WINDOW + 1:]),
    ]
    return cases


def golden_inputs():
    """Every input of tests/golden/index_cases.json as (name, spec, bytes);
    spec is {'hex': ...} for a crafted input of up to 512 bytes, {'crafted':
    name} for a larger one and {'gen': [kind, n, seed]} for a generated one.
    The bom_* inputs are raw file bytes: decoded() gives the bytes indexed."""
    out = []
    sample = "h\u00e9llo w\u00f6rld, \u20acuro \u4e2d\u6587 \U0001f600 index\n"
    for name, raw in (("bom_utf8", b"\xef\xbb\xbf" + sample.encode()),
                      ("bom_utf8_only", b"\xef\xbb\xbf"),
                      ("bom_utf16le", b"\xff\xfe" + sample.encode("utf-16-le")),
                      ("bom_utf16be", b"\xfe\xff" + sample.encode("utf-16-be")),
                      ("bom_utf32le", b"\xff\xfe\x00\x00" + sample.encode("utf-32-le")),
                      ("bom_utf32be", b"\x00\x00\xfe\xff" + sample.encode("utf-32-be"))):
        out.append((name, {"hex": raw.hex()}, raw))
    for name, data in crafted_flag_cases():
        spec = {"hex": data.hex()} if len(data) <= 512 else {"crafted": name}
        out.append(("flag_" + name, spec, data))
    gens = [("words", 0, 1), ("words", 1, 1), ("words", 2, 1), ("ascii", 7, 2), ("ascii", 8, 2), ("ascii", 9, 2),
            ("words", 15, 3), ("words", 16, 3), ("words", 17, 3), ("words", 4096, 6), ("words", 65537, 8),
            ("random", 131072, 9), ("repeat", 70000, 0xFF), ("repeat", 777, 0x61), ("random", 1 << 20, 11),
            ("words", 800001, 12)]
    for kind, n, seed in gens:
        out.append(("gen_%s_%d_%d" % (kind, n, seed), {"gen": [kind, n, seed]}, gen_input(kind, n, seed)))
    return out


def decoded(raw):
    """The bytes reflex::Input delivers for a file: a UTF-8 BOM dropped,
    UTF-16/32 with a BOM converted (transcode_model.direct)."""
    import transcode_model as tm
    raw = bytes(raw)
    enc, skip = tm.detect_bom(raw[:4], len(raw))
    return raw[skip:] if enc in (tm.PLAIN, tm.UTF8) else tm.direct(raw[skip:], enc)


def input_of(spec):
    if "hex" in spec:
        return bytes.fromhex(spec["hex"])
    if "crafted" in spec:
        return dict(crafted_flag_cases())[spec["crafted"]]
    return gen_input(*spec["gen"])
