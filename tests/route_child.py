"""Child process of tests/test_route.py: runs every case with UGPU_TRACE=1 (the
parent sets it: the switch is cached per process) and prints one JSON line
{case: {"got": ..., "want": ..., ...}} on stdout.  Before each case it writes a
marker line "[case] name" to stderr, where the engine's trace lines go, so the
parent can tell which steps a case ran.  Inputs are at most 64 KiB."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

N = 64 << 10
FIRST = ["foo|bar|baz", "[A-Za-z_][A-Za-z0-9_]*", r"\w+", "a+", "x[a-z]*y", r"\d+\.\d+", "(ab)+", "[a-z]+ing", r"\S+",
         ".", "words300", r"\w+ \w+"]
IDENT = "[A-Za-z_][A-Za-z0-9_]*"


def mark(name):
    os.write(2, ("[case] %s\n" % name).encode())


def inputs():
    import numpy as np
    from oracle_lib import gen
    words = gen(1, 53, 0, N)                       # ASCII words
    # Devanagari: the lead E0 A4 is XU_MIX for \w (letters, signs and digits share its
    # block beyond the three continuation classes, tables.hpp): the fast U kernel flags it
    deva = np.frombuffer("  अआइ कखग ०१ ।  ".encode(), np.uint8)
    mixed = words.copy()
    mixed[10000:10000 + deva.size] = deva
    four = words.copy()
    four[30000:30008] = np.frombuffer(b"  " + "\U0001d400".encode() + b"  ", np.uint8)  # U+1D400, a Word letter
    stray = words.copy()
    stray[20000:20016] = ord(" ")
    stray[20004:20007] = np.frombuffer(b"x\x80a", np.uint8)  # (tests/test_word.py: at_wb looks back past the stray byte)
    code = gen(3, 19, 0, N)                        # ASCII source code
    high = code.copy()
    high[40000] = 0xe9
    return dict(words=words, utf8=gen(4, 17, 0, N), mixed=mixed, four=four, stray=stray, code=code, high=high)


def main():
    import torch

    import ugrep_amd as U
    import wordset_gen
    from oracle_lib import OracleDfa
    ins = inputs()
    dev = {k: torch.from_numpy(v).to("cuda") for k, v in ins.items()}
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    out = {}

    def oracle(opc, word, data, want_list=False):
        o = OracleDfa(opc)
        r = o.find_w(data, want_list=want_list) if word else o.find(data, want_list=want_list)
        return [r[0], r[1], r[2]] + ([r[3]] if want_list else [])

    def scan(name, pat, opc, word, inp, sc=None):
        """One ugpu_scan + ugpu_scan_totals of the whole input on a scanner of its own (or sc)."""
        sc = sc or U.Scanner(pat)
        mark(name)
        sc.scan(dev[inp].data_ptr(), 0, N, N, True, 0, st)
        t = sc.totals()
        out[name] = dict(kernel=pat.info()["kernel"], got=[t.count, t.digest, t.dcap], flags=t.flags,
                         want=oracle(opc, word, ins[inp]))
        return sc

    for rx in FIRST:
        opc = U.compile_regex(wordset_gen.regex(wordset_gen.words(300)) if rx == "words300" else rx)
        for word in (False, True):
            scan("first|%s|w%d" % (rx, word), U.Pattern(opc, word=word), opc, word, "utf8")

    wopc, iopc = U.compile_regex(r"\w+"), U.compile_regex(IDENT)
    wp, wpw, ipw = U.Pattern(wopc), U.Pattern(wopc, word=True), U.Pattern(iopc, word=True)
    scan("redo|w+|clean", wp, wopc, False, "words")
    sc = scan("redo|w+|mixed", wp, wopc, False, "mixed")
    scan("redo|w+|mixed again", wp, wopc, False, "mixed", sc)
    scan("redo|w+|four", wp, wopc, False, "four")
    scan("redo|-w w+|clean", wpw, wopc, True, "words")
    scan("redo|-w w+|stray", wpw, wopc, True, "stray")
    scan("redo|-w ident|ascii", ipw, iopc, True, "code")
    scan("redo|-w ident|high", ipw, iopc, True, "high")

    # OFFSETS after an xi COUNT (the route knobs are read when the scanner is created)
    os.environ["UGPU_XC"] = os.environ["UGPU_XU"] = "0"
    try:
        pat = U.Pattern(iopc)
        mark("offsets|ident")
        res = U.find_all(pat, dev["code"], offsets=True)
        out["offsets|ident"] = dict(kernel=pat.info()["kernel"], got=[res.count, res.digest, res.dcap, res.triples()],
                                    want=oracle(iopc, False, ins["code"], want_list=True))
    finally:
        os.environ.pop("UGPU_XC")
        os.environ.pop("UGPU_XU")
    mark("end")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
