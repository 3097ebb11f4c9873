"""Child process of tests/test_ws_growth.py: the growth paths of the pooled
workspaces, which in the long-lived test process run only by accident of test
order (the pools live as long as the process).  In a fresh process every step
below starts from empty or smaller buffers.  Prints one JSON line; the parent
compares it with the oracle.  Inputs are at most 2 MiB.

The order matters: steps 1 and 2 use a table with few matches (c2_foobarbaz), so
the record lists they leave behind are short and step 3's sub-batch outgrows
them while it holds records (the keep-growth)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

MIB = 1 << 20
FIND_SIZES = [4 << 10, 64 << 10, MIB, 4 << 10]
FEEDS = [1 << 10, 1 << 10, MIB + MIB // 2]  # then the rest of STREAM_LEN
STREAM_LEN = 2 * MIB
KEEP = 4096
BATCH_PATTERN = "\\w+$"  # (tests/golden/anchor_cases.json: reads its line context)
BATCH_CR = 40            # the input that ends in a bare CR
REC_SIZES = [256 << 10, 2 * MIB]
UTF8_SIZES = [1 << 10, MIB]


def tables():
    """opc of c2_foobarbaz, c3_ident and the line-context fixture."""
    cfg = json.load(open(os.path.join(os.path.dirname(HERE), "ugrep_amd", "data", "config_patterns.json")))
    anchor = json.load(open(os.path.join(HERE, "golden", "anchor_cases.json")))["cases"]
    return dict(c2=cfg["c2_foobarbaz"]["opc"], c3=cfg["c3_ident"]["opc"],
                eol=next(c for c in anchor if c["pattern"] == BATCH_PATTERN and not c["nul"])["opc"])


def inputs():
    from oracle_lib import gen
    planted = gen(2, 7, 0, STREAM_LEN)   # foo / bar / baz planted in words
    words = gen(1, 31, 0, MIB)
    batch, off = [], 0
    for i in range(64):                  # 256 B to 8 KiB, ascending
        n = 256 + i * (8192 - 256) // 63
        d = words[off:off + n].tobytes()
        off += n
        if i == BATCH_CR:
            d = d[:-1] + b"\r"
        batch.append(d)
    utf8 = []
    for n in UTF8_SIZES:
        d = gen(4, 17, 0, n).copy()
        d[n - 5] = 0xff                  # one bad byte near the end
        utf8.append(d)
    return dict(planted=planted, batch=batch, code=gen(3, 19, 0, REC_SIZES[-1]), utf8=utf8)


def main():
    import torch

    import ugrep_amd as U
    ins, tab = inputs(), tables()
    out = {}

    def lst(r):
        return [r.count, r.digest, r.dcap, r.triples()]

    # 1. find_all on growing host inputs, then the smallest again (no shrink)
    c2 = U.Pattern(tab["c2"])
    out["find_all"] = [lst(U.find_all(c2, ins["planted"][:n], offsets=True)) for n in FIND_SIZES]

    # 2. one stream whose third feed outgrows the first buffers while a carry is held
    s = U.Stream(c2, keep=KEEP)
    rows, count, at = [], 0, 0
    for n in FEEDS + [STREAM_LEN - sum(FEEDS)]:
        r = s.feed(ins["planted"][at:at + n], final=at + n == STREAM_LEN)
        at += n
        count += r.count
        rows += r.triples()
    s.close()
    out["stream"] = [count, rows]

    # 3. a batch served input by input (line context and a bare CR): its record lists grow while they hold records
    eol = U.Pattern(tab["eol"])
    res = U.find_batch(eol, ins["batch"], offsets=True)
    out["batch"] = dict(contexts=eol.info()["contexts"], one_scan=res.one_scan, count=res.count,
                        got=[lst(res.input(i)[0]) for i in range(len(ins["batch"]))],
                        find_all=[lst(U.find_all(eol, d, offsets=True)) for d in ins["batch"]])

    # 4. records of 256 KiB, then of 2 MiB
    c3 = U.Pattern(tab["c3"])
    out["records"] = []
    for n in REC_SIZES:
        r = U.Records(c3, ins["code"][:n])
        out["records"].append(list(r.drain()))
        r.close()

    # 5. the binary tests on device buffers
    out["utf8"] = []
    for d in ins["utf8"]:
        t = torch.from_numpy(d).to("cuda")
        torch.cuda.synchronize()
        out["utf8"].append(dict(first_bad=U.check_utf8(t.data_ptr(), d.size), binary=U.is_binary(t.data_ptr(), d.size),
                                nul=U.find_nul(t.data_ptr(), d.size)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
