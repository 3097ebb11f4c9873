#!/usr/bin/env python3
"""Regenerate tests/golden/transcode_cases.json and
tests/golden/transcode_inputs.bin (run in the build container only).

Input-conversion goldens from the REFERENCE's CLI, which prints the converted
stream line by line (and one '\\n' more when the stream does not end in one):

  cases   oracle/_ref/ugrep --no-config -a [--encoding=NAME] '' FILE, the raw
          output recorded per case, for the three lorem files of
          tests/golden/verify/ and for crafted inputs (below), which are kept
          back to back in transcode_inputs.bin ([offset, length] per case);
  pages   the CP1252 and KOI8-R tables, recovered from the CLI's output over
          the input  x b \\n  for b = 0..255 (256 values each: data);
  bom     one head per row of Input::file_init's BOM table with the encoding
          and the skip it announces; where the row announces a conversion the
          CLI's output over the head is recorded too;
  words   the rows of  -ob '\\w+'  over the three lorem files ([offset, byte
          length]), and the count of  -iwco -f lorem  for each.

UTF-16/32 cases carry a BOM, so no forced-encoding head is involved; Latin-1
and page cases begin with an ASCII byte other than NUL.

Usage: make -C oracle ref && python tests/golden/make_transcode_golden.py
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
UGREP = os.path.join(REPO, "oracle", "_ref", "ugrep")
sys.path.insert(0, os.path.join(REPO, "tests"))
import transcode_model as M  # noqa: E402

BOMS = {"utf16le": b"\xff\xfe", "utf16be": b"\xfe\xff", "utf32le": b"\xff\xfe\x00\x00", "utf32be": b"\x00\x00\xfe\xff"}
PAGES = {"cp1252": "CP1252", "koi8r": "KOI8-R"}


def cli(args, path):
    return subprocess.run([UGREP, "--no-config"] + args + [path], stdout=subprocess.PIPE, check=False).stdout


def cli_bytes(args, data):
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(data)
        f.flush()
        return cli(args, f.name)


def u16(order, *units):
    return b"".join(struct.pack("<H" if order == "le" else ">H", u) for u in units)


def u32(order, *vals):
    return b"".join(struct.pack("<I" if order == "le" else ">I", v & 0xFFFFFFFF) for v in vals)


def utf16_cases(order):
    """(name, payload) list"""
    A, NL, X = 0x41, 0x0A, 0x78
    body = []
    for run in range(1, 6):                      # H-runs followed by a low surrogate and by a BMP unit
        hs = [0xD800 + 7 * k + run for k in range(run)]
        body += hs + [0xDC00 + run, X, NL]
        body += hs + [0x20AC, X, NL]
        body += hs + [A, A, X, NL]
    body += [0xDC00, X, NL, 0xDFFF, 0xDC01, X, NL]                      # lone low surrogates
    body += [0xD83D, 0xDE00, 0xD800, 0xDC00, 0xDBFF, 0xDFFF, X, NL]     # valid pairs
    body += [0xE9, 0x7FF, 0x800, 0x20AC, 0xFFFF, 0x7F, 0x80, NL]
    out = [("body", u16(order, *body))]
    for run in range(1, 6):                      # H-runs that end the input
        out.append(("run%d_end" % run, u16(order, A, NL, *[0xDA00 + k for k in range(run)])))
    tails = {"tail0": b"", "tail1": b"\x41", "tail2_low": u16(order, 0xDC05), "tail2_bmp": u16(order, A),
             "tail3_low": u16(order, 0xDC05) + b"\x41", "tail3_bmp": u16(order, A) + b"\xdc"}
    for name, t in tails.items():                # bytes behind a final H
        out.append((name, u16(order, A, X, NL, 0xD801) + t))
    out.append(("odd", u16(order, A, X, NL, 0xE9) + b"\xd8"))
    return out


def utf32_cases(order):
    vals = [0x7F, 0x80, 0x7FF, 0x800, 0xD800, 0xFFFF, 0x10000, 0x10FFFF, 0x110000, 0x7FFFFFFF, 0x80000041, 0xFFFFFFFF]
    body = []
    for v in vals:
        body += [0x78, v, 0x0A]
    out = [("body", u32(order, *body))]
    for k in (1, 2, 3):
        out.append(("tail%d" % k, u32(order, 0x41, 0x0A, 0xE9) + b"\x41\x00\x00"[:k]))
    return out


def parse_page(out):
    """page[b] from the CLI's output over  x b \\n  for b = 0..255"""
    page, i = [], 0
    for b in range(256):
        assert out[i] == 0x78, (b, i)
        c = out[i + 1]
        n = 1 if c < 0x80 else 2 if c < 0xE0 else 3 if c < 0xF0 else 4
        seq = out[i + 1:i + 1 + n]
        cp = c if n == 1 else int.from_bytes(seq.decode("utf-8", "surrogatepass").encode("utf-32-le", "surrogatepass"),
                                             "little")
        assert M.utf8(cp) == seq, (b, seq)
        assert out[i + 1 + n] == 0x0A, (b, i)
        page.append(cp)
        i += n + 2
    assert i == len(out)
    assert page[0x0A] == 0x0A and page.count(0x0A) == 1
    return page


def main():
    if not os.path.exists(UGREP):
        sys.exit("build the reference CLI first: make -C oracle ref")
    blob, cases = bytearray(), []

    def add(name, enc, data, args=()):
        out = cli_bytes(["-a"] + list(args) + [""], data)
        cases.append(dict(name=name, enc=enc, input=[len(blob), len(data)], args=list(args), out=out.hex()))
        blob.extend(data)

    for fname, enc, args in (("lorem.utf16.txt", "bom", []), ("lorem.utf32.txt", "bom", []),
                             ("lorem.latin1.txt", "latin1", ["--encoding=LATIN1"])):
        out = cli(["-a"] + args + [""], os.path.join(HERE, "verify", fname))
        cases.append(dict(name=fname, enc=enc, file="verify/" + fname, args=args, out=out.hex()))
    for order in ("le", "be"):
        for name, payload in utf16_cases(order):
            add("utf16%s_%s" % (order, name), "bom", BOMS["utf16" + order] + payload)
        for name, payload in utf32_cases(order):
            add("utf32%s_%s" % (order, name), "bom", BOMS["utf32" + order] + payload)
    add("latin1_all", "latin1", b"x" + bytes(range(256)) + b"\n", ["--encoding=LATIN1"])
    add("null_data", "null_data", b"x\x00ab\ncd\x00\x00\n\nef", ["--encoding=null-data"])
    pages = {}
    probe = b"".join(b"x" + bytes([b]) + b"\n" for b in range(256))
    for key, name in PAGES.items():
        add("page_" + key, "page:" + key, probe, ["--encoding=" + name])
        pages[key] = parse_page(bytes.fromhex(cases[-1]["out"]))

    bom = []
    heads = [(b"\xef\xbb\xbfA\n", "utf8", 3), (b"\xfe\xff\x00A\x00\n", "utf16be", 2),
             (b"\xff\xfe\x00\x00A\x00\x00\x00\n\x00\x00\x00", "utf32le", 4), (b"\xff\xfeA\x00\n\x00", "utf16le", 2),
             (b"\xff\xfeA", "plain", 0), (b"\xff\xfe", "plain", 0), (b"\x00\x00\xfe\xff\x00\x00\x00A\x00\x00\x00\n", "utf32be", 4),
             (b"\xfe\xff", "utf16be", 2), (b"ab\n", "plain", 0), (b"\xef\xbbA\n", "plain", 0), (b"", "plain", 0)]
    for head, enc, skip in heads:
        row = dict(head=head.hex(), enc=enc, skip=skip)
        if enc not in ("plain",) and len(head) > skip:
            row["out"] = cli_bytes(["-a", ""], head).hex()
        bom.append(row)

    words = {}
    for fname, args in (("lorem.utf16.txt", []), ("lorem.utf32.txt", []), ("lorem.latin1.txt", ["--encoding=LATIN1"])):
        path = os.path.join(HERE, "verify", fname)
        rows = []
        for ln in cli(["-ob"] + args + [r"\w+"], path).split(b"\n"):
            if ln:
                off, _, w = ln.partition(b":")
                rows.append([int(off), len(w)])
        pat = open(os.path.join(HERE, "verify", "lorem"), "rb").read()
        cnt = subprocess.run([UGREP, "--no-config", "-iwco"] + args + ["-f", "-", path], input=pat,
                             stdout=subprocess.PIPE, check=True).stdout
        words[fname] = dict(args=args, rows=rows, iwco=int(cnt))

    with open(os.path.join(HERE, "transcode_inputs.bin"), "wb") as f:
        f.write(bytes(blob))
    with open(os.path.join(HERE, "transcode_cases.json"), "w") as fh:
        json.dump(dict(source="ugrep --no-config -a [--encoding=NAME] '' FILE; -ob '\\w+' FILE; -iwco -f lorem FILE",
                       inputs="transcode_inputs.bin", cases=cases, pages=pages, bom=bom, words=words), fh,
                  separators=(",", ":"))
    print("cases", len(cases), "input bytes", len(blob), "words", {k: len(v["rows"]) for k, v in words.items()},
          "iwco", {k: v["iwco"] for k, v in words.items()})


if __name__ == "__main__":
    main()
