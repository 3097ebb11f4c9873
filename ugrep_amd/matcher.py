"""Host-side mirror of the reference matcher interface for the FIND hot path.

    reflex::Pattern(const Opcode *code, ...)   include/reflex/pattern.h:151-159
    reflex::Matcher(pattern); m.buffer(base, size); while (m.find()) ...
        find  = AbstractMatcher::Operation, include/reflex/absmatcher.h:276-280, :1401
        first = absmatcher.h:901-905, size = :651-658, accept = :605-609

`Pattern` takes the compiled opcode words (Pattern::opc_) and uploads the dense
tables once; `Matcher` serves find() from one whole-buffer GPU scan, the way a
ugrep worker consumes matches from a mmap'd file (src/ugrep.cpp:3936-3940,
:10544).  Everything runs through the HIP engine (libugrep_amd.so); there is no
CPU fallback in this module: tables the engine does not support raise
`Unsupported`, as ugpu_dfa_create returns UGPU_UNSUPPORTED.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import BIN_INIT_WINDOW, BIN_NUL_ONLY, BIN_NULL_DATA, check, lib


def _as_u32(opc):
    a = np.ascontiguousarray(np.asarray(opc, dtype=np.uint32))
    return a, a.ctypes.data_as(_lib.c_u32p)


RX_FIXED = 1
RX_ICASE = 2
RX_REFLEX = 4
PAT_WORD = 1  # ugpu_dfa_create pattern_flags: option W
PAT_EMPTY = 2  # ugpu_dfa_create pattern_flags: option N (empty matches)


def compile_regex(regex, fixed=False, icase=False, reflex=False):
    """Opcode words (numpy u32) for `regex` from the native compiler
    (ugpu_compile, regex_compile.cpp): ugrep's default ERE in Unicode mode, as
    Matcher::convert(rx, notnewline|unicode) + Pattern(conv, "r") produce them
    (src/ugrep.cpp:8574-8578, lib/pattern.cpp:171-3063).  Syntax errors raise
    UgpuError(UGPU_INVAL) where the reference throws regex_error; constructs the
    GPU tables do not cover raise Unsupported.  reflex=True: `regex` is the
    RE/flex byte regex a Pattern holds after ugrep's conversion
    (Pattern::operator[](0), UGPU_RX_REFLEX), as the drop-in adapter passes it."""
    if isinstance(regex, str):
        regex = regex.encode("utf-8")
    words = _lib.c_u32p()
    n = ctypes.c_uint32()
    flags = (RX_FIXED if fixed else 0) | (RX_ICASE if icase else 0) | (RX_REFLEX if reflex else 0)
    rc = lib.ugpu_compile(regex, len(regex), flags, ctypes.byref(words), ctypes.byref(n))
    if rc != _lib.UGPU_OK:
        msg = lib.ugpu_compile_error().decode(errors="replace")
        raise (_lib.Unsupported if rc == _lib.UGPU_UNSUPPORTED else _lib.UgpuError)(rc, msg)
    try:
        return np.ctypeslib.as_array(words, shape=(n.value,)).copy()
    finally:
        lib.ugpu_opc_free(words)


def host_tables(opc):
    """Dense tables built on the host (no device needed): dict of numpy arrays."""
    a, p = _as_u32(opc)
    info = _lib.DfaInfo()
    check(lib.ugpu_tables_build_host(p, len(a), ctypes.byref(info), None, 0, None, None, 0, None, None))
    trans = np.zeros(info.states * info.row, np.uint16)
    cls = np.zeros(256, np.uint8)
    caps = np.zeros(info.states, np.uint32)
    start = ctypes.c_uint32()
    accb = ctypes.c_uint32()
    check(lib.ugpu_tables_build_host(p, len(a), ctypes.byref(info), trans.ctypes.data_as(_lib.c_u16p), len(trans),
                                     cls.ctypes.data_as(_lib.c_u8p), caps.ctypes.data_as(_lib.c_u32p), len(caps),
                                     ctypes.byref(start), ctypes.byref(accb)))
    return dict(info={f: getattr(info, f) for f, _ in _lib.DfaInfo._fields_}, trans=trans, cls=cls, caps=caps,
                start=start.value, accb=accb.value)


def host_context(opc):
    """(acap u32[states * 4], anchored, start_acc): the per-context accept
    indices acap[state * 4 + bol * 2 + eol] of the dense tables (tables.hpp)."""
    a, p = _as_u32(opc)
    info = _lib.DfaInfo()
    check(lib.ugpu_tables_build_host(p, len(a), ctypes.byref(info), None, 0, None, None, 0, None, None))
    acap = np.zeros(info.states * max(info.contexts, 4), np.uint32)
    an, sa = ctypes.c_int(), ctypes.c_int()
    check(lib.ugpu_tables_context_host(p, len(a), acap.ctypes.data_as(_lib.c_u32p), len(acap), ctypes.byref(an),
                                       ctypes.byref(sa)))
    return acap, bool(an.value), bool(sa.value)


def host_prefilter(opc):
    """(enabled, ft[20]) prefilter lookup tables built on the host (tables.hpp)."""
    a, p = _as_u32(opc)
    ft = np.zeros(20, np.uint8)
    en = ctypes.c_int()
    check(lib.ugpu_tables_prefilter_host(p, len(a), ft.ctypes.data_as(_lib.c_u8p), ctypes.byref(en)))
    return bool(en.value), ft


def host_plan(opc, word=False, empty=False):
    """The info dict Pattern(opc, word, empty).info() would report (kernel
    choice included), decided on the host without a device
    (ugpu_dfa_plan_host); raises like Pattern() for unsupported tables."""
    a, p = _as_u32(compile_regex(opc) if isinstance(opc, (str, bytes)) else opc)
    info = _lib.DfaInfo()
    check(lib.ugpu_dfa_plan_host(p, len(a), (PAT_WORD if word else 0) | (PAT_EMPTY if empty else 0),
                                 ctypes.byref(info)))
    return {f: getattr(info, f) for f, _ in _lib.DfaInfo._fields_}


def host_transducer(opc):
    """FIND transducer table (u16 numpy array, tables.hpp) or None when the DFA
    is not restart-local."""
    a, p = _as_u32(opc)
    t = host_tables(opc)
    x = np.zeros(t["info"]["states"] * t["info"]["row"], np.uint16)
    loc = ctypes.c_int()
    check(lib.ugpu_tables_transducer_host(p, len(a), x.ctypes.data_as(_lib.c_u16p), len(x), ctypes.byref(loc)))
    return x if loc.value else None


def host_immediate(opc):
    """Immediate transducer of xi_kernel: (xid table as uint8[rows, 256], sync byte) or None."""
    a, p = _as_u32(opc)
    rows, sb, imm = ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_int()
    check(lib.ugpu_tables_immediate_host(p, len(a), None, 0, ctypes.byref(rows), ctypes.byref(sb), ctypes.byref(imm)))
    if not imm.value:
        return None
    x = np.zeros(rows.value * 256, np.uint8)
    check(lib.ugpu_tables_immediate_host(p, len(a), x.ctypes.data_as(_lib.c_u8p), x.size, ctypes.byref(rows),
                                         ctypes.byref(sb), ctypes.byref(imm)))
    return x.reshape(rows.value, 256), sb.value


def host_gap(opc):
    """Gap transducer of xg_kernel: (xg table uint16[states*row], sync uint8[256]) or None."""
    a, p = _as_u32(opc)
    info = host_tables(opc)["info"]
    x = np.zeros(info["states"] * info["row"], np.uint16)
    sy = np.zeros(256, np.uint8)
    ok = ctypes.c_int()
    check(lib.ugpu_tables_gap_host(p, len(a), x.ctypes.data_as(_lib.c_u16p), x.size, sy.ctypes.data_as(_lib.c_u8p),
                                   ctypes.byref(ok)))
    return (x, sy) if ok.value else None


def host_equivalent(opc_a, opc_b):
    """True when two opcode tables accept the same strings with the same accept indices."""
    a, pa = _as_u32(opc_a)
    b, pb = _as_u32(opc_b)
    eq = ctypes.c_int(0)
    check(lib.ugpu_tables_equivalent_host(pa, len(a), pb, len(b), ctypes.byref(eq)))
    return bool(eq.value)


def host_xc(opc):
    """Byte classes of xc_kernel (two-state tables): cls uint8[256] = G << 7 | X << 6, or None."""
    a, p = _as_u32(opc)
    ok = ctypes.c_int(0)
    cls = np.zeros(256, np.uint8)
    check(lib.ugpu_tables_xc_host(p, len(a), cls.ctypes.data_as(_lib.c_u8p), ctypes.byref(ok)))
    return cls if ok.value else None


def host_xu(opc):
    """Code-point run tables of xc_kernel's U mode: (tab uint8[16896], bm3 uint32[2048]), or None."""
    a, p = _as_u32(opc)
    ok = ctypes.c_int(0)
    tab = np.zeros(256 + 64 * 256 + 256, np.uint8)  # (tables.hpp kXuTab)
    bm3 = np.zeros(2048, np.uint32)
    check(lib.ugpu_tables_xu_host(p, len(a), tab.ctypes.data_as(_lib.c_u8p), bm3.ctypes.data_as(_lib.c_u32p),
                                  ctypes.byref(ok)))
    return (tab, bm3) if ok.value else None


def host_dom(opc, want_all=False):
    """Dominated-restart bits of the dense tables (tables.hpp dom): a bool
    numpy array over state ids (ugpu_tables_build_host numbering), or None
    when they were not computed; want_all: (bits, dom_all)."""
    a, p = _as_u32(opc)
    n = ctypes.c_uint32(0)
    al = ctypes.c_int(0)
    check(lib.ugpu_tables_dom_host(p, len(a), None, 0, ctypes.byref(n), ctypes.byref(al)))
    bits = None
    if n.value:
        w = np.zeros(n.value, np.uint32)
        check(lib.ugpu_tables_dom_host(p, len(a), w.ctypes.data_as(_lib.c_u32p), n.value, ctypes.byref(n), None))
        bits = np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)
    return (bits, bool(al.value)) if want_all else bits


def host_ngram(opc, word=False):
    """The n-gram candidate filter of kernel 7 (ngram.hpp, ugpu_tables_ngram_host),
    built on the host: dict(n, log2_bits, bitmap uint32[2^log2_bits / 32], ppm,
    fill, enabled), or None when the table has none.  ppm = the estimated
    candidate positions per million on text, fill = the bitmap's share of set
    bits, enabled = the plan takes kernel 7 under `word`."""
    a, p = _as_u32(compile_regex(opc) if isinstance(opc, (str, bytes)) else opc)
    fl = PAT_WORD if word else 0
    n, k, ppm, en = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
    check(lib.ugpu_tables_ngram_host(p, len(a), fl, ctypes.byref(n), ctypes.byref(k), None, 0, ctypes.byref(ppm),
                                     ctypes.byref(en)))
    if not n.value:
        return None
    bm = np.zeros((1 << k.value) // 32, np.uint32)
    check(lib.ugpu_tables_ngram_host(p, len(a), fl, ctypes.byref(n), ctypes.byref(k), bm.ctypes.data_as(_lib.c_u32p),
                                     len(bm), ctypes.byref(ppm), ctypes.byref(en)))
    fill = float(np.unpackbits(bm.view(np.uint8)).sum()) / float(1 << k.value)
    return dict(n=n.value, log2_bits=k.value, bitmap=bm, ppm=ppm.value, fill=fill, enabled=bool(en.value))


def host_ngram_candidates(opc, data, word=False):
    """uint8[len(data)]: 1 where the n-gram filter, as the device evaluates it
    over the whole buffer, makes the position a candidate
    (ugpu_ngram_candidates_host)."""
    a, p = _as_u32(compile_regex(opc) if isinstance(opc, (str, bytes)) else opc)
    buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data,
                               dtype=np.uint8)
    out = np.zeros(len(buf), np.uint8)
    check(lib.ugpu_ngram_candidates_host(p, len(a), PAT_WORD if word else 0, buf.ctypes.data_as(_lib.c_u8p), len(buf),
                                         out.ctypes.data_as(_lib.c_u8p)))
    return out


class Pattern:
    """Compiled pattern (opcode words) with its device tables."""

    def __init__(self, opc, word=False, empty=False):
        """opc: opcode words (or a regex for compile_regex).  word=True is
        Matcher option W (ugrep -w, reflex::Matcher(pat, input, "W"),
        src/ugrep.cpp:8616-8618): whole-buffer scans on wfind_kernel.
        empty=True is option N (ugrep -Y, -x): empty matches are reported."""
        if isinstance(opc, (str, bytes)):
            opc = compile_regex(opc)
        self.opc, p = _as_u32(opc)
        self.word = bool(word)
        self.empty = bool(empty)
        h = ctypes.c_void_p()
        check(lib.ugpu_dfa_create(p, len(self.opc), (PAT_WORD if word else 0) | (PAT_EMPTY if empty else 0),
                                  ctypes.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def info(self):
        info = _lib.DfaInfo()
        check(lib.ugpu_dfa_info_get(self._h, ctypes.byref(info)))
        return {f: getattr(info, f) for f, _ in _lib.DfaInfo._fields_}

    def close(self):
        if getattr(self, "_h", None):
            lib.ugpu_dfa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _buffer_ptr(data):
    """(pointer, length, keepalive) of bytes / numpy / torch (host or device) data."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        return arr.ctypes.data, arr.size, arr
    if isinstance(data, np.ndarray):
        arr = np.ascontiguousarray(data.view(np.uint8).reshape(-1))
        return arr.ctypes.data, arr.size, arr
    if hasattr(data, "data_ptr"):  # torch tensor, host or device
        t = data.contiguous()
        return t.data_ptr(), t.numel() * t.element_size(), t
    raise TypeError("unsupported buffer type %r" % type(data))


class FindResult:
    def __init__(self, count, digest, dcap, start=None, length=None, cap=None):
        self.count, self.digest, self.dcap = count, digest, dcap
        self.start, self.length, self.cap = start, length, cap

    def triples(self):
        return [[int(s), int(l), int(c)] for s, l, c in zip(self.start, self.length, self.cap)]


def _take_result(res, offsets):
    try:
        r = res.contents
        if offsets and r.count:
            st = np.ctypeslib.as_array(r.start, shape=(r.count,)).copy()
            ln = np.ctypeslib.as_array(r.len, shape=(r.count,)).copy()
            cp = np.ctypeslib.as_array(r.cap, shape=(r.count,)).copy()
        else:
            st = np.zeros(0, np.uint64)
            ln = np.zeros(0, np.uint32)
            cp = np.zeros(0, np.uint32)
        return FindResult(r.count, r.digest, r.dcap, st, ln, cp)
    finally:
        lib.ugpu_result_free(res)


def find_all(pattern, data, start=0, offsets=True):
    """ugpu_find_all: every FIND match of `data` from position `start`."""
    ptr, n, keep = _buffer_ptr(data)
    res = ctypes.POINTER(_lib.Result)()
    check(lib.ugpu_find_all(pattern.handle, ctypes.c_void_p(ptr), n, start,
                            _lib.MODE_OFFSETS if offsets else _lib.MODE_COUNT, ctypes.byref(res)))
    out = _take_result(res, offsets)
    del keep
    return out


def find_all_multi(pattern, data, ndev=0, start=0, offsets=True):
    """ugpu_find_all_multi: as find_all, with [start, len) cut into ndev shards
    at arbitrary offsets, shard k on device k mod the visible devices (ndev 0:
    one per device), chains resolved across the cuts."""
    ptr, n, keep = _buffer_ptr(data)
    res = ctypes.POINTER(_lib.Result)()
    check(lib.ugpu_find_all_multi(pattern.handle, ctypes.c_void_p(ptr), n, start,
                                  _lib.MODE_OFFSETS if offsets else _lib.MODE_COUNT, ndev, ctypes.byref(res)))
    out = _take_result(res, offsets)
    del keep
    return out


class Records:
    """ugpu_find_records: the records of a buffer for a one-at-a-time consumer
    (pipelined H2D, scans and packed record copy-back; include/ugpu.h)."""

    def __init__(self, pattern, data, start=0, borrow=False):
        """borrow=True (UGPU_REC_BORROW): this object keeps `data` alive until
        close(), and the first records can be popped while the rest of the
        input is still on its way to the device."""
        ptr, n, keep = _buffer_ptr(data)
        h = ctypes.c_void_p()
        if borrow:
            check(lib.ugpu_find_records_ex(pattern.handle, ctypes.c_void_p(ptr), n, start, 1, ctypes.byref(h)))
            self._keep = (keep, data)
        else:
            check(lib.ugpu_find_records(pattern.handle, ctypes.c_void_p(ptr), n, start, ctypes.byref(h)))
            del keep
        self._h = h

    def next(self):
        """(start, len, cap) of the next record, or None."""
        s, ln, c = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        rc = lib.ugpu_records_next(self._h, ctypes.byref(s), ctypes.byref(ln), ctypes.byref(c))
        if rc < 0:
            check(-rc)
        return (s.value, ln.value, c.value) if rc == 1 else None

    def triples(self):
        out = []
        while True:
            t = self.next()
            if t is None:
                return out
            out.append(list(t))

    def totals(self):
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.ugpu_records_totals(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def drain(self):
        """Pop every remaining record natively: (n, digest, dcap)."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.ugpu_records_drain(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def close(self):
        if getattr(self, "_h", None):
            lib.ugpu_records_free(self._h)
            self._h = None
        self._keep = None  # (a borrowed buffer outlives the pipeline)

    def __del__(self):
        self.close()


class Stream:
    """Streaming FIND over input fed in chunks (ugpu_stream):
    feed() returns the matches that became final, with absolute offsets."""

    def __init__(self, pattern, keep=0):
        self.pattern = pattern
        h = ctypes.c_void_p()
        check(lib.ugpu_stream_create(pattern.handle, keep, ctypes.byref(h)))
        self._h = h

    def feed(self, chunk, final=False, offsets=True, flush=False):
        """final: the input ends here; flush: more may follow, but settle every
        match the bytes so far decide (UGPU_FEED_FLUSH: an input that would block)."""
        ptr, n, keep = _buffer_ptr(chunk)
        res = ctypes.POINTER(_lib.Result)()
        check(lib.ugpu_stream_feed(self._h, ctypes.c_void_p(ptr), n, 1 if final else (2 if flush else 0),
                                   _lib.MODE_OFFSETS if offsets else _lib.MODE_COUNT, ctypes.byref(res)))
        out = _take_result(res, offsets)
        del keep
        return out

    def settled(self):
        return lib.ugpu_stream_settled(self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib.ugpu_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Matcher:
    """FIND over a fully buffered input: m = Matcher(pat, data); while m.find(): m.first(), m.size()."""

    def __init__(self, pattern, data=None):
        self.pattern = pattern
        self._data = None
        if data is not None:
            self.buffer(data)

    def buffer(self, data):
        """AbstractMatcher::buffer(base, size): whole input, cursor at 0 (absmatcher.h:542-591)."""
        self._data = data
        self._cur = 0
        self._from = 0
        self._res = None
        self._i = 0
        self._first = 0
        self._size = 0
        self._cap = 0
        return self

    def _inside_match(self):
        """The cursor lies strictly inside a record of the current scan."""
        r, i = self._res, max(self._i - 1, 0)
        while i < r.count and int(r.start[i]) + int(r.length[i]) <= self._cur:
            i += 1
        return i < r.count and int(r.start[i]) < self._cur

    def find(self):
        """Next match at or after the cursor; returns its accept index, 0 when exhausted.

        The FIND chain passes through every position that is not strictly
        inside one of its matches, so after skip_to() the remaining records
        stay exact unless the cursor landed inside a match; then (as the C++
        adapter, integration/reflex_gpu_matcher.h) the scan is re-run from the
        cursor."""
        if self._res is None or self._cur < self._from or self._inside_match():
            self._res = find_all(self.pattern, self._data, self._cur, offsets=True)
            self._from = self._cur
            self._i = 0
        r = self._res
        while self._i < r.count and int(r.start[self._i]) < self._cur:
            self._i += 1
        if self._i >= r.count:
            self._cap = 0
            self._size = 0
            return 0
        self._first = int(r.start[self._i])
        self._size = int(r.length[self._i])
        self._cap = int(r.cap[self._i])
        self._cur = self._first + self._size
        self._i += 1
        return self._cap

    def first(self):
        return self._first

    def size(self):
        return self._size

    def last(self):
        return self._first + self._size

    def accept(self):
        return self._cap

    def skip_to(self, pos):
        """Advance the cursor (the effect of skip('\\n') on cur_ between finds)."""
        self._cur = max(self._cur, pos)

    def __iter__(self):
        while self.find():
            yield self._first, self._size, self._cap


class Scanner:
    """Device-resident scans (ugpu_scanner): one per stream/thread."""

    def __init__(self, pattern, records=False):
        """records=True: scans will be followed by offsets() -- prefer kernels
        with their own record pass (UGPU_SCANNER_RECORDS)."""
        self.pattern = pattern
        h = ctypes.c_void_p()
        check(lib.ugpu_scanner_create_ex(pattern.handle, 1 if records else 0, ctypes.byref(h)))
        self._h = h

    def scan(self, dptr, lo, hi, read_end=None, at_eof=True, bias=0, stream=0):
        if read_end is None:
            read_end = hi
        check(lib.ugpu_scan(self._h, ctypes.c_void_p(dptr), lo, hi, read_end, 1 if at_eof else 0, bias,
                            ctypes.c_void_p(stream)))

    def totals(self):
        t = _lib.Totals()
        check(lib.ugpu_scan_totals(self._h, ctypes.byref(t)))
        return t

    def context(self, bol0):
        """ugpu_scanner_context: whether dbuf[0] begins a line (anchored tables)."""
        check(lib.ugpu_scanner_context(self._h, 1 if bol0 else 0))

    def stage(self, on=True):
        """Single-pass OFFSETS: COUNT scans stage the records of prefiltered tables."""
        check(lib.ugpu_scanner_stage(self._h, 1 if on else 0))

    def kernel_ms(self):
        ms = ctypes.c_float()
        check(lib.ugpu_scan_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def offsets(self, d_start, d_len, d_cap, capacity, stream=0):
        """Write the last scan's records; d_cap 0/None: 12-byte records (tables
        with one accept index, info()["shape"] & SHAPE_ONE_ACCEPT)."""
        check(lib.ugpu_scan_offsets(self._h, ctypes.c_void_p(d_start), ctypes.c_void_p(d_len),
                                    ctypes.c_void_p(d_cap or None), capacity, ctypes.c_void_p(stream)))

    def chain_fix(self, dptr, lo, hi, read_end, at_eof, bias, old_entry, new_entry, stream=0):
        t = _lib.Totals()
        check(lib.ugpu_chain_fix(self._h, ctypes.c_void_p(dptr), lo, hi, read_end, 1 if at_eof else 0, bias,
                                 old_entry, new_entry, ctypes.byref(t), ctypes.c_void_p(stream)))
        return t

    def close(self):
        if getattr(self, "_h", None):
            lib.ugpu_scanner_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lines(dptr, length, d_start=0, n=0, d_line=0, stream=0):
    """ugpu_lines over a 16-byte aligned device buffer: (newlines, matching_lines);
    fills d_line[i] with the 1-based line of d_start[i] when d_line is given."""
    nl = ctypes.c_uint64()
    ml = ctypes.c_uint64()
    check(lib.ugpu_lines(ctypes.c_void_p(dptr), length, ctypes.c_void_p(d_start), n, ctypes.c_void_p(d_line),
                         ctypes.byref(nl), ctypes.byref(ml), ctypes.c_void_p(stream)))
    return nl.value, ml.value


def columns(dptr, length, d_pos, n, tab=8, d_col=0, d_bol=0, d_line=0, stream=0):
    """ugpu_columns over a 16-byte aligned device buffer and an ascending device
    list of n positions in [0, length]: fills d_col[i] with the 0-based column
    of d_pos[i] (ugrep -k prints it plus 1; `tab` is --tabs: 1, 2, 4 or 8),
    d_bol[i] with the begin of its line and d_line[i] with its 1-based line.
    Each output may be 0, not all three."""
    check(lib.ugpu_columns(ctypes.c_void_p(dptr), length, ctypes.c_void_p(d_pos or None), n, tab,
                           ctypes.c_void_p(d_col or None), ctypes.c_void_p(d_bol or None),
                           ctypes.c_void_p(d_line or None), ctypes.c_void_p(stream)))


PositionResult = collections.namedtuple("PositionResult", "line column start length cap")


def find_positions(pattern, data, tab=8):
    """The rows of `ugrep -onkb --tabs=tab` for one input:
    PositionResult(line, column, start, length, cap) numpy arrays, one entry
    per match; line is 1-based, column 0-based (ugrep prints column + 1), start
    the byte offset.  Composes find_all and columns; the column work runs on
    the current device."""
    import torch
    ptr, n, keep = _buffer_ptr(data)
    dev = _device_input(ptr, n, keep)
    r = find_all(pattern, dev[:n], offsets=True)
    m = int(r.count)
    out = torch.zeros((2, max(m, 1)), dtype=torch.int64, device=dev.device)
    if m:
        d_pos = torch.from_numpy(r.start.astype(np.int64)).to(dev.device)
        torch.cuda.synchronize()
        columns(dev.data_ptr(), n, d_pos.data_ptr(), m, tab, d_col=out[0].data_ptr(), d_line=out[1].data_ptr())
    col, line = (a.astype(np.uint64) for a in out[:, :m].cpu().numpy())
    del keep
    return PositionResult(line, col, r.start, r.length, r.cap)


def select_lines(dptr, length, d_start, d_len, n, invert=False, d_begin=0, d_end=0, d_lineno=0, capacity=0,
                 stream=0):
    """ugpu_select_lines over a 16-byte aligned device buffer and its sorted
    device match list (d_len 0: zero-length matches): (selected, lines).  The
    records (begin, end, lineno) of the lines the matches touch (invert: of the
    others) go to the three device arrays of `capacity` elements (all 0: count
    only).  Too small a capacity raises UgpuError with code UGPU_CAPACITY and
    the counts in its .selected / .lines."""
    sel = ctypes.c_uint64()
    nl = ctypes.c_uint64()
    rc = lib.ugpu_select_lines(ctypes.c_void_p(dptr), length, ctypes.c_void_p(d_start or None),
                               ctypes.c_void_p(d_len or None), n, _lib.SEL_INVERT if invert else 0,
                               ctypes.c_void_p(d_begin or None), ctypes.c_void_p(d_end or None),
                               ctypes.c_void_p(d_lineno or None), capacity, ctypes.byref(sel), ctypes.byref(nl),
                               ctypes.c_void_p(stream))
    if rc == _lib.UGPU_CAPACITY:
        err = _lib.UgpuError(rc, lib.ugpu_last_error().decode(errors="replace"))
        err.selected, err.lines = sel.value, nl.value
        raise err
    check(rc)
    return sel.value, nl.value


def line_spans(dptr, length, d_lineno, n, d_begin, d_end, stream=0):
    """ugpu_line_spans: d_begin[i], d_end[i] = byte span (newline excluded) of
    line d_lineno[i] of an ascending device list; 2^64-1 in both for a line
    that does not exist."""
    check(lib.ugpu_line_spans(ctypes.c_void_p(dptr), length, ctypes.c_void_p(d_lineno or None), n,
                              ctypes.c_void_p(d_begin or None), ctypes.c_void_p(d_end or None),
                              ctypes.c_void_p(stream)))


def context_lines(selected_lineno, nlines, before, after):
    """The lines ugrep prints for -B before -A after around the selected lines
    (ascending, 1-based) of an input of nlines lines: (lineno, kind), merged and
    ascending, kind 1 = selected, 0 = context; context is clipped to the input."""
    sel = np.asarray(selected_lineno, dtype=np.int64)
    if sel.size == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint8)
    lo = np.maximum(sel - int(before), 1)
    hi = np.minimum(sel + int(after), int(nlines))
    new = np.ones(sel.size, bool)  # a group begins where the window leaves a gap behind the previous one
    new[1:] = lo[1:] > hi[:-1] + 1
    first = np.flatnonzero(new)
    glo = lo[first]
    ghi = hi[np.append(first[1:] - 1, sel.size - 1)]
    cnt = ghi - glo + 1
    off = np.cumsum(cnt) - cnt
    lineno = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(off, cnt) + np.repeat(glo, cnt)
    at = np.searchsorted(sel, lineno)
    kind = (sel[np.minimum(at, sel.size - 1)] == lineno).astype(np.uint8)
    return lineno.astype(np.uint64), kind


LineResult = collections.namedtuple("LineResult", "lineno begin end kind")


def grep_lines(pattern, data, invert=False, before=0, after=0):
    """The lines `ugrep -n [-v] [-B before] [-A after]` prints for one input:
    LineResult(lineno, begin, end, kind) numpy arrays, ascending; data[begin:end]
    is the line without its newline, kind 1 = selected, 0 = context.  Composes
    find_all, select_lines, context_lines and, for the context lines only,
    line_spans; the line work runs on the current device."""
    import torch
    ptr, n, keep = _buffer_ptr(data)
    if n == 0:  # an empty input has no lines
        return _no_lines()
    dev = _device_input(ptr, n, keep)
    d_start, d_len, m = _device_matches(pattern, dev, n)
    torch.cuda.synchronize()
    sel, nlines = select_lines(dev.data_ptr(), n, d_start.data_ptr(), d_len.data_ptr(), m, invert)
    rec = torch.zeros((3, max(sel, 1)), dtype=torch.int64, device=dev.device)
    torch.cuda.synchronize()
    select_lines(dev.data_ptr(), n, d_start.data_ptr(), d_len.data_ptr(), m, invert, rec[0].data_ptr(),
                 rec[1].data_ptr(), rec[2].data_ptr(), sel)
    out = _with_context(dev, n, rec, sel, nlines, before, after)
    del keep
    return out


def _no_lines():
    return LineResult(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint8))


def _device_input(ptr, n, keep):
    """The input as a 16-byte aligned device tensor, readable to the end of its
    last granule (the line kernels load whole granules)."""
    import torch
    if hasattr(keep, "is_cuda") and keep.is_cuda and not ptr & 15:
        return keep.view(torch.uint8).reshape(-1)
    dev = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    if n:
        src = keep if hasattr(keep, "data_ptr") else torch.from_numpy(keep if keep.flags.writeable else keep.copy())
        dev[:n].copy_(src.view(torch.uint8).reshape(-1))
    return dev


def _device_matches(pattern, dev, n):
    """(d_start, d_len, count): the match list of dev[:n] as device tensors."""
    import torch
    r = find_all(pattern, dev[:n], offsets=True)
    d_start = torch.from_numpy(r.start.astype(np.int64)).to(dev.device)
    d_len = torch.from_numpy(r.length.astype(np.int32)).to(dev.device)
    return d_start, d_len, int(r.count)


def _with_context(dev, n, rec, sel, nlines, before, after):
    """LineResult of the `sel` records in the device tensor rec[3][>= sel]
    (begin, end, lineno) plus their context lines (line_spans)."""
    import torch
    begin, end, lineno = (a.astype(np.uint64) for a in rec[:, :sel].cpu().numpy())
    kind = np.ones(sel, np.uint8)
    if (before or after) and sel:
        lineno_all, kind = context_lines(lineno, nlines, before, after)
        ctx = kind == 0
        nctx = int(ctx.sum())
        b_all = np.empty(lineno_all.size, np.uint64)
        e_all = np.empty(lineno_all.size, np.uint64)
        b_all[~ctx], e_all[~ctx] = begin, end
        if nctx:
            q = torch.from_numpy(lineno_all[ctx].astype(np.int64)).to(dev.device)
            sp = torch.zeros((2, nctx), dtype=torch.int64, device=dev.device)
            torch.cuda.synchronize()
            line_spans(dev.data_ptr(), n, q.data_ptr(), nctx, sp[0].data_ptr(), sp[1].data_ptr())
            b_all[ctx], e_all[ctx] = (a.astype(np.uint64) for a in sp.cpu().numpy())
        lineno, begin, end = lineno_all, b_all, e_all
    return LineResult(lineno, begin, end, kind)


def select_lines_bool(dptr, length, lists, clauses, invert=False, files=False, d_begin=0, d_end=0, d_lineno=0,
                      capacity=0, stream=0):
    """ugpu_select_lines_bool over a 16-byte aligned device buffer:
    (selected, lines, whole).  `lists` is a sequence of (d_start, d_len, n)
    sorted device match lists (d_len 0: zero-length matches; an empty list may
    have null pointers), `clauses` a sequence of (pos, neg) bit masks over
    them: a line is selected when every clause has a pos list that touches it
    or a neg list that does not.  files=True (--files) evaluates the lists over
    the whole input and selects the lines any list touches when the formula
    holds; `whole` is then the formula's value.  Records and capacity as
    select_lines."""
    lists = list(lists)
    clauses = list(clauses)
    k, nc = len(lists), len(clauses)
    starts = (ctypes.c_void_p * max(k, 1))(*[ctypes.c_void_p(int(a[0]) or None) for a in lists])
    lens = (ctypes.c_void_p * max(k, 1))(*[ctypes.c_void_p(int(a[1]) or None) for a in lists])
    counts = (ctypes.c_uint64 * max(k, 1))(*[int(a[2]) for a in lists])
    cl = (_lib.BoolClause * max(nc, 1))(*[_lib.BoolClause(int(p), int(q)) for p, q in clauses])
    sel = ctypes.c_uint64()
    nl = ctypes.c_uint64()
    whole = ctypes.c_int()
    flags = (_lib.SEL_INVERT if invert else 0) | (_lib.BOOL_FILES if files else 0)
    rc = lib.ugpu_select_lines_bool(ctypes.c_void_p(dptr), length, starts, lens, counts, k, cl, nc, flags,
                                    ctypes.c_void_p(d_begin or None), ctypes.c_void_p(d_end or None),
                                    ctypes.c_void_p(d_lineno or None), capacity, ctypes.byref(sel), ctypes.byref(nl),
                                    ctypes.byref(whole), ctypes.c_void_p(stream))
    if rc == _lib.UGPU_CAPACITY:
        err = _lib.UgpuError(rc, lib.ugpu_last_error().decode(errors="replace"))
        err.selected, err.lines = sel.value, nl.value
        raise err
    check(rc)
    return sel.value, nl.value, bool(whole.value)


def host_newline(opc):
    """ugpu_tables_newline_host: whether some match of the table can contain '\\n'."""
    a, p = _as_u32(opc)
    nl = ctypes.c_int()
    check(lib.ugpu_tables_newline_host(p, len(a), ctypes.byref(nl)))
    return bool(nl.value)


# --- batched FIND (ugpu_find_batch; replaces the per-file loop, src/ugrep.cpp:4261-4480) ---

def host_batch_plan(opc, word=False, empty=False):
    """ugpu_batch_plan_host: whether a batch on this table is served by one
    scan of the packed inputs (no match can contain '\\n', no option N);
    raises like Pattern() for unsupported tables."""
    a, p = _as_u32(compile_regex(opc) if isinstance(opc, (str, bytes)) else opc)
    one = ctypes.c_int()
    check(lib.ugpu_batch_plan_host(p, len(a), (PAT_WORD if word else 0) | (PAT_EMPTY if empty else 0),
                                   ctypes.byref(one)))
    return bool(one.value)


def split_matches(dptr, length, d_bounds, nseg, d_start, d_len, d_cap, cap1, n, d_first, d_digest, d_dcap,
                  d_newlines, d_mlines, d_rel=0, d_line=0, stream=0):
    """ugpu_split_matches over a 16-byte aligned device buffer, its sorted
    device match list (d_len 0: zero lengths; d_cap 0: every accept index is
    cap1) and nseg + 1 ascending device bounds: fills the per-segment device
    arrays d_first (nseg + 1), d_digest, d_dcap, d_newlines, d_mlines (nseg) and,
    when given, the per-record d_rel and d_line."""
    v = ctypes.c_void_p
    check(lib.ugpu_split_matches(v(dptr), length, v(d_bounds), nseg, v(d_start or None), v(d_len or None),
                                 v(d_cap or None), cap1, n, v(d_first), v(d_digest or None), v(d_dcap or None),
                                 v(d_newlines or None), v(d_mlines or None), v(d_rel or None), v(d_line or None),
                                 v(stream)))


class BatchResult:
    """Per-input results of find_batch: input i owns the records
    [first[i], first[i+1]); start is relative to its input, line is the 1-based
    line within it; start, length, cap and line are None without offsets."""

    def __init__(self, one_scan, count, first, digest, dcap, newlines, matching_lines, start=None, length=None,
                 cap=None, line=None):
        self.one_scan, self.count, self.first = one_scan, count, first
        self.digest, self.dcap, self.newlines, self.matching_lines = digest, dcap, newlines, matching_lines
        self.start, self.length, self.cap, self.line = start, length, cap, line

    def __len__(self):
        return len(self.digest)

    def input(self, i):
        """(FindResult, line slice) of input i."""
        a, b = int(self.first[i]), int(self.first[i + 1])
        if self.start is None:
            return FindResult(b - a, int(self.digest[i]), int(self.dcap[i]), np.zeros(0, np.uint64),
                              np.zeros(0, np.uint32), np.zeros(0, np.uint32)), None
        return FindResult(b - a, int(self.digest[i]), int(self.dcap[i]), self.start[a:b], self.length[a:b],
                          self.cap[a:b]), self.line[a:b]


def find_batch(pattern, inputs, offsets=True):
    """ugpu_find_batch: FIND over a sequence of host inputs (bytes, numpy or
    host tensors) in one packed scan where the table allows it; every input's
    results equal find_all and lines over that input alone."""
    bufs = [_buffer_ptr(d) for d in inputs]
    k = len(bufs)
    ptrs = (ctypes.c_void_p * max(k, 1))(*[b[0] if b[1] else None for b in bufs])
    lens = np.array([b[1] for b in bufs], dtype=np.uint64)
    res = ctypes.POINTER(_lib.BatchResult)()
    check(lib.ugpu_find_batch(pattern.handle, ptrs, lens.ctypes.data_as(_lib.c_u64p), k,
                              _lib.MODE_OFFSETS if offsets else _lib.MODE_COUNT, ctypes.byref(res)))
    try:
        r = res.contents

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dt)

        out = BatchResult(bool(r.flags & _lib.BATCH_ONE_SCAN), r.count, arr(r.first, k + 1, np.uint64),
                          arr(r.digest, k, np.uint64), arr(r.dcap, k, np.uint64), arr(r.newlines, k, np.uint64),
                          arr(r.matching_lines, k, np.uint64))
        if offsets:
            out.start = arr(r.start, r.count, np.uint64)
            out.length = arr(r.len, r.count, np.uint32)
            out.cap = arr(r.cap, r.count, np.uint32)
            out.line = arr(r.line, r.count, np.uint64)
    finally:
        lib.ugpu_batch_free(res)
    del bufs
    return out


# --- ugrep --bool queries (grammar: src/cnf.hpp:227-237) ---
#   and  -> or { space+ [ 'AND' space+ ] or }*
#   or   -> not { ( '|'+ | 'OR' space+ ) not }*
#   not  -> [ '-' space* | 'NOT' space+ ] atom
#   atom -> '(' and ')' | pattern
# A '(' opens a group only when it is not '(?' and its ')' is followed by the
# end, a space, '|' or ')' (so (foo|bar)? stays one pattern); a pattern runs
# to the next space, '|' or ')' outside its own parentheses, brackets, quotes
# and escapes; "..." is a literal (\Q...\E).

def _skip_unit(s, i):
    """Index behind the bracket list, quoted string, escape, \\Q..\\E span or
    single character at s[i]."""
    c = s[i]
    if c == "[":
        j = i + 1
        if j < len(s) and s[j] == "^":
            j += 1
        if j < len(s):
            j += 1  # a leading ] is a member
        while j < len(s) and s[j] != "]":
            j += 2 if s[j] == "\\" and j + 1 < len(s) else 1
        return min(j + 1, len(s))
    if c == '"':
        j = i + 1
        while j < len(s) and s[j] != '"':
            j += 2 if s[j] == "\\" and j + 1 < len(s) else 1
        return min(j + 1, len(s))
    if c == "\\":
        if s.startswith("\\Q", i):
            j = s.find("\\E", i + 2)
            return len(s) if j < 0 else j + 2
        return min(i + 2, len(s))
    return i + 1


def _is_space(s, i):
    return i < len(s) and s[i] in " \t\r\f\v"


class _BoolParser:
    def __init__(self, s):
        if "\n" in s:
            raise ValueError("a newline in a Boolean query is not supported")
        self.s, self.i = s, 0
        self.patterns = []

    def space(self):
        while _is_space(self.s, self.i):
            self.i += 1

    def word(self, w):
        """Consume operator word w when it stands here followed by a space."""
        if self.s.startswith(w, self.i) and _is_space(self.s, self.i + len(w)):
            self.i += len(w)
            self.space()
            return True
        return False

    def parse_and(self):
        items = []
        self.space()
        while self.i < len(self.s) and self.s[self.i] != ")":
            items.append(self.parse_or())
            self.space()
            self.word("AND")
        return ("and", items)

    def parse_or(self):
        items = [self.parse_not()]
        while True:
            j = self.i
            self.space()
            if self.i < len(self.s) and self.s[self.i] == "|":
                while self.i < len(self.s) and self.s[self.i] == "|":
                    self.i += 1
                self.space()
            elif not self.word("OR"):
                self.i = j
                return ("or", items)
            items.append(self.parse_not())

    def parse_not(self):
        s = self.s
        neg = False
        if self.i < len(s) and s[self.i] == "-":
            neg = True
            self.i += 1
            self.space()
        elif self.word("NOT"):
            neg = True
        node = self.parse_atom()
        return ("not", node) if neg else node

    def group_end(self):
        """Index of the ')' closing the '(' at self.i when that pair is a group, else -1."""
        s, j, level = self.s, self.i + 1, 0
        if s.startswith("(?", self.i):
            return -1
        while j < len(s):
            if s[j] == "(":
                level += 1
            elif s[j] == ")":
                if level == 0:
                    k = j + 1
                    return j if k == len(s) or s[k] in "|)" or _is_space(s, k) else -1
                level -= 1
            j = _skip_unit(s, j)
        return -1

    def parse_atom(self):
        s = self.s
        if self.i < len(s) and s[self.i] == "(":
            end = self.group_end()
            if end >= 0:
                self.i += 1
                node = self.parse_and()
                if self.i != end:
                    raise ValueError("unbalanced parentheses in Boolean query at offset %d" % self.i)
                self.i += 1
                if not node[1]:
                    raise ValueError("empty group in Boolean query")
                return node
        out, level = "", 0
        while self.i < len(s):
            c = s[self.i]
            if level == 0 and (c in "|)" or _is_space(s, self.i)):
                break
            j = _skip_unit(s, self.i)
            if c == '"':
                closed = j - 1 > self.i and s[j - 1] == '"'
                lit = s[self.i + 1:j - 1 if closed else j].replace('\\"', '"')
                if lit:
                    out += "\\Q" + lit.replace("\\E", "\\E\\\\E\\Q") + "\\E"
            else:
                if c == "(":
                    level += 1
                elif c == ")":
                    level -= 1
                out += s[self.i:j]
            self.i = j
        if level:
            raise ValueError("unbalanced parentheses in Boolean query")
        if not out:
            raise ValueError("empty pattern in Boolean query at offset %d" % self.i)
        if out not in self.patterns:
            self.patterns.append(out)
        return ("lit", self.patterns.index(out))


def _cnf(node, neg, limit):
    """Clauses [(pos, neg)] of the tree `node` (complemented when neg): NOT is
    pushed to the leaves (De Morgan), OR distributes over AND; clauses holding
    a pattern and its complement are true and dropped, repeats are dropped."""
    kind = node[0]
    if kind == "lit":
        return [(0, 1 << node[1])] if neg else [(1 << node[1], 0)]
    if kind == "not":
        return _cnf(node[1], not neg, limit)
    parts = [_cnf(ch, neg, limit) for ch in node[1]]
    out = []
    if (kind == "and") != neg:  # a conjunction: the clauses of every part
        for p in parts:
            for c in p:
                if c not in out:
                    out.append(c)
    else:  # a disjunction: one clause per choice of a clause from every part
        out = [(0, 0)]
        for p in parts:
            nxt = []
            for a in out:
                for b in p:
                    c = (a[0] | b[0], a[1] | b[1])
                    if not (c[0] & c[1]) and c not in nxt:
                        nxt.append(c)
            out = nxt
            if len(out) > 64 * limit:
                raise ValueError("Boolean query needs more than %d clauses" % limit)
    return out


def parse_bool_query(query):
    """(patterns, clauses) of a ugrep --bool query: space or AND means and, |
    or OR means or, - or NOT means not (NOT binds tighter than OR, OR tighter
    than AND), parentheses group, "..." is a literal.  The query is normalised
    to CNF: `clauses` is a list of (pos, neg) bit masks over `patterns` (equal
    pattern strings share one entry), as select_lines_bool takes them; the
    empty query gives no clause.  ValueError for more than 16 distinct
    patterns, more than 64 clauses, or a construct outside this grammar."""
    p = _BoolParser(query)
    tree = p.parse_and()
    if p.i != len(query):
        raise ValueError("unbalanced ')' in Boolean query at offset %d" % p.i)
    if len(p.patterns) > _lib.BOOL_MAX_LISTS:
        raise ValueError("Boolean query has more than %d distinct patterns" % _lib.BOOL_MAX_LISTS)
    clauses = _cnf(tree, False, _lib.BOOL_MAX_CLAUSES)
    if len(clauses) > _lib.BOOL_MAX_CLAUSES:
        raise ValueError("Boolean query needs more than %d clauses" % _lib.BOOL_MAX_CLAUSES)
    return p.patterns, clauses


def _expand_quotes(rx):
    r"""`rx` with every \Q...\E span written as escaped characters (the native
    compiler has no \Q)."""
    out, i = "", 0
    while i < len(rx):
        if rx.startswith("\\Q", i):
            j = rx.find("\\E", i + 2)
            j = len(rx) if j < 0 else j
            out += "".join("\\" + c if c in "\\.^$*+?()[]{}|" else c for c in rx[i + 2:j])
            i = j + 2
        elif rx[i] == "\\" and i + 1 < len(rx):
            out += rx[i:i + 2]
            i += 2
        else:
            out += rx[i]
            i += 1
    return out


def grep_bool(query_or_cnf, data, invert=False, files=False, before=0, after=0, icase=False):
    """The lines `ugrep -n --bool QUERY [-v] [--files] [-B before] [-A after]`
    prints for one input, as grep_lines returns them.  query_or_cnf is a --bool
    query string (parse_bool_query) or a (patterns, clauses) pair: -e A --and B
    --andnot C is (["A", "B", "C"], [(1, 0), (2, 0), (0, 4)]).  Every pattern is
    compiled (compile_regex) and scanned once over the one device copy of the
    input (find_all), then select_lines_bool picks the lines.  A pattern that
    can match a newline raises ValueError: the per-line semantics of the
    reference differ for it (include/ugpu.h)."""
    import torch
    patterns, clauses = parse_bool_query(query_or_cnf) if isinstance(query_or_cnf, str) else query_or_cnf
    pats = []
    for rx in patterns:
        opc = compile_regex(_expand_quotes(rx), icase=icase)
        if host_newline(opc):
            raise ValueError("pattern %r can match a newline: not supported in a Boolean line query" % (rx,))
        pats.append(Pattern(opc))
    ptr, n, keep = _buffer_ptr(data)
    if n == 0:  # an empty input has no lines
        return _no_lines()
    dev = _device_input(ptr, n, keep)
    found = [_device_matches(p, dev, n) for p in pats]
    lists = [(s.data_ptr() if m else 0, ln.data_ptr() if m else 0, m) for s, ln, m in found]
    # without a pattern the reference's primary pattern is empty and matches every line, --files or not
    files = bool(files) and bool(pats)
    torch.cuda.synchronize()
    sel, nlines, _ = select_lines_bool(dev.data_ptr(), n, lists, clauses, invert, files)
    rec = torch.zeros((3, max(sel, 1)), dtype=torch.int64, device=dev.device)
    torch.cuda.synchronize()
    select_lines_bool(dev.data_ptr(), n, lists, clauses, invert, files, rec[0].data_ptr(), rec[1].data_ptr(),
                      rec[2].data_ptr(), sel)
    out = _with_context(dev, n, rec, sel, nlines, before, after)
    del keep, found
    return out


def check_utf8(dptr, length, stream=0):
    """reflex::isutf8 over device bytes (ugpu_check_utf8): None when valid,
    else the offset of the first failing byte (length for a cut-off sequence)."""
    r = ctypes.c_uint64()
    check(lib.ugpu_check_utf8(ctypes.c_void_p(dptr), length, ctypes.byref(r), ctypes.c_void_p(stream)))
    return None if r.value == 0xFFFFFFFFFFFFFFFF else r.value


def isutf8(dptr, length, stream=0):
    """reflex::isutf8(s, s + length) (lib/simd.cpp:169) on a device buffer."""
    return check_utf8(dptr, length, stream) is None


def find_nul(dptr, length, stream=0):
    """memchr(s, '\\0', length) on a device buffer: offset or None."""
    r = ctypes.c_uint64()
    check(lib.ugpu_find_nul(ctypes.c_void_p(dptr), length, ctypes.byref(r), ctypes.c_void_p(stream)))
    return None if r.value == 0xFFFFFFFFFFFFFFFF else r.value


def is_binary(dptr, length, null_data=False, nul_only=False, init_window=False, stream=0):
    """ugrep's is_binary (src/ugrep.cpp:699-711); init_window adds
    init_is_binary's trailing-sequence trim (:3998-4015)."""
    flags = (BIN_NULL_DATA if null_data else 0) | (BIN_NUL_ONLY if nul_only else 0) | \
        (BIN_INIT_WINDOW if init_window else 0)
    r = ctypes.c_int()
    check(lib.ugpu_is_binary(ctypes.c_void_p(dptr), length, flags, ctypes.byref(r), ctypes.c_void_p(stream)))
    return bool(r.value)


def gen(kind, seed, off, dptr, length, stream=0):
    """Generate corpus bytes [off, off+length) on the device (ugpu_gen)."""
    check(lib.ugpu_gen(kind, seed, off, ctypes.c_void_p(dptr), length, ctypes.c_void_p(stream)))


# ---- input encodings (ugpu_detect_bom, ugpu_transcode)

# the names of ugrep's --encoding= that have no code page (src/ugrep.cpp:4497-4541), lower case
ENCODINGS = {"utf-8": _lib.ENC_UTF8, "utf-16be": _lib.ENC_UTF16BE, "utf-16le": _lib.ENC_UTF16LE, "utf-16": _lib.ENC_UTF16BE,
             "utf-32be": _lib.ENC_UTF32BE, "utf-32le": _lib.ENC_UTF32LE, "utf-32": _lib.ENC_UTF32BE,
             "latin1": _lib.ENC_LATIN1, "iso-8859-1": _lib.ENC_LATIN1, "null-data": _lib.ENC_NULL_DATA}


def detect_bom(head, length=None):
    """Input::file_init's BOM checks (ugpu_detect_bom): (enc, skip) for an
    input of `length` bytes (default: len(head)) whose first bytes are `head`."""
    head = bytes(head[:4])
    n = len(head) if length is None else int(length)
    buf = (ctypes.c_uint8 * 4)(*head[:min(n, 4)])
    enc, skip = ctypes.c_uint32(), ctypes.c_uint32()
    check(lib.ugpu_detect_bom(buf, n, ctypes.byref(enc), ctypes.byref(skip)))
    return enc.value, skip.value


def transcode_bound(enc, nbytes):
    """ugpu_transcode_bound: the largest output of nbytes input bytes under enc."""
    b = ctypes.c_uint64()
    check(lib.ugpu_transcode_bound(enc, nbytes, ctypes.byref(b)))
    return b.value


def transcode(dptr, length, enc, start=0, page=None, d_dst=0, capacity=0, stream=0):
    """ugpu_transcode: converts the device bytes [start, length) of a 16-byte
    aligned buffer from `enc` (a _lib.ENC_* value; `page`: the 256 values of a
    code page for ENC_PAGE) into the 16-byte aligned device buffer d_dst of
    `capacity` bytes and returns the output length; d_dst 0 only asks for that
    length.  Too small a capacity raises UgpuError with code UGPU_CAPACITY and
    the length in its .out_len; nothing is written then."""
    out = ctypes.c_uint64()
    pg = None if page is None else (ctypes.c_uint16 * 256)(*[int(x) for x in page])
    rc = lib.ugpu_transcode(ctypes.c_void_p(dptr), length, start, enc, pg, ctypes.c_void_p(d_dst or None), capacity,
                            ctypes.byref(out), ctypes.c_void_p(stream))
    if rc == _lib.UGPU_CAPACITY:
        err = _lib.UgpuError(rc, lib.ugpu_last_error().decode(errors="replace"))
        err.out_len = out.value
        raise err
    check(rc)
    return out.value


def decode_input(data, encoding=None, page=None):
    """Host bytes as the UTF-8 (or plain) device bytes the scans and line
    consumers take, as reflex::Input hands them to the matcher: (device uint8
    tensor, n).  The tensor is 16-byte aligned and holds a zeroed granule
    behind its n bytes.  Without `encoding` the BOM decides (detect_bom; none:
    the bytes as they are); `encoding` is a name of ENCODINGS or an ENC_* value,
    and a `page` (256 values) selects ENC_PAGE.  A BOM is skipped only when it
    was detected, not under a given encoding."""
    import torch
    _, n, keep = _buffer_ptr(data)
    host = keep if isinstance(keep, np.ndarray) else keep.view(torch.uint8).reshape(-1).cpu().numpy()
    skip = 0
    if page is not None:
        enc = _lib.ENC_PAGE
    elif encoding is None:
        enc, skip = detect_bom(host[:4].tobytes() if n else b"", n)
    else:
        enc = ENCODINGS[encoding.lower()] if isinstance(encoding, str) else int(encoding)
    if enc in (_lib.ENC_PLAIN, _lib.ENC_UTF8):
        dev = torch.zeros(n - skip + 16, dtype=torch.uint8, device="cuda")
        if n - skip:
            dev[:n - skip].copy_(torch.from_numpy(host[skip:].copy()))
        del keep
        return dev, n - skip
    src = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    if n:
        src[:n].copy_(torch.from_numpy(host.copy()))
    torch.cuda.synchronize()
    m = transcode(src.data_ptr(), n, enc, skip, page)
    dst = torch.zeros(m + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = transcode(src.data_ptr(), n, enc, skip, page, dst.data_ptr(), m)
    assert got == m
    del keep
    return dst, m


def find_encoded(pattern, data, encoding=None, page=None, offsets=True):
    """find_all over decode_input(data, encoding, page): the matches of an
    input in another encoding; the offsets are positions in the converted
    stream, as ugrep -b prints them."""
    dev, n = decode_input(data, encoding, page)
    return find_all(pattern, dev[:n], offsets=offsets)


# ---- file indexes (ugpu_index_tables, ugpu_index_batch): ugrep-indexer's pass

INDEX_MAGIC = b"UG#\x03\x00"
INDEX_STORE = "._UG#_Store"


class IndexResult:
    """Per-input results of index_batch: header[i] is the record's second byte
    (log2 of the table size, bit 7: binary), zero_bits[i] the zero bits of the
    final table, and input i's table is tables[offset[i]:offset[i+1]]."""

    def __init__(self, accuracy, header, zero_bits, offset, tables):
        self.accuracy, self.header, self.zero_bits, self.offset, self.tables = accuracy, header, zero_bits, offset, tables

    def __len__(self):
        return len(self.header)

    def table(self, i):
        return self.tables[int(self.offset[i]):int(self.offset[i + 1])].tobytes()

    def binary(self, i):
        return bool(self.header[i] & 0x80)

    def noise_percent(self, i):
        """What ugrep-indexer -v prints for the input."""
        size = int(self.offset[i + 1]) - int(self.offset[i])
        return int(100.0 * int(self.zero_bits[i]) / (8 * size) + 0.5) if size else 0


def index_chunk():
    """ugpu_index_chunk: the bytes of an input one workgroup hashes."""
    return int(lib.ugpu_index_chunk())


def index_tables(dptr, length, bounds, accuracy=4, ignore_binary=False, d_tables=0, capacity=0, stream=0):
    """ugpu_index_tables over the segments [bounds[s], bounds[s+1]) of a 16-byte
    aligned device buffer: (header, zero_bits, offset, tables_len) with the
    tables written to the device buffer d_tables of `capacity` bytes (0: a size
    query).  Too small a capacity raises UgpuError (UGPU_CAPACITY) with the
    length in its .out_len."""
    b = np.ascontiguousarray(bounds, dtype=np.uint64)
    nseg = b.size - 1
    header = np.zeros(nseg + 1, np.uint8)
    zeros = np.zeros(nseg + 1, np.uint32)
    offset = np.zeros(nseg + 1, np.uint64)
    total = ctypes.c_uint64()
    rc = lib.ugpu_index_tables(ctypes.c_void_p(dptr or None), length, b.ctypes.data_as(_lib.c_u64p), nseg, accuracy,
                               _lib.INDEX_IGNORE_BINARY if ignore_binary else 0, header.ctypes.data_as(_lib.c_u8p),
                               zeros.ctypes.data_as(_lib.c_u32p), offset.ctypes.data_as(_lib.c_u64p),
                               ctypes.c_void_p(d_tables or None), capacity, ctypes.byref(total), ctypes.c_void_p(stream))
    if rc == _lib.UGPU_CAPACITY:
        err = _lib.UgpuError(rc, lib.ugpu_last_error().decode(errors="replace"))
        err.out_len = total.value
        raise err
    check(rc)
    return header[:nseg], zeros[:nseg], offset, total.value


def index_batch(inputs, accuracy=4, ignore_binary=False):
    """ugpu_index_batch: the index records of a sequence of host inputs (bytes,
    numpy or host tensors), each as ugrep-indexer -ACCURACY [-I] computes it for
    a file of those bytes: an IndexResult."""
    bufs = [_buffer_ptr(d) for d in inputs]
    k = len(bufs)
    ptrs = (ctypes.c_void_p * max(k, 1))(*[b[0] if b[1] else None for b in bufs])
    lens = np.array([b[1] for b in bufs], dtype=np.uint64)
    res = ctypes.POINTER(_lib.IndexResult)()
    check(lib.ugpu_index_batch(ptrs, lens.ctypes.data_as(_lib.c_u64p), k, accuracy,
                               _lib.INDEX_IGNORE_BINARY if ignore_binary else 0, ctypes.byref(res)))
    try:
        r = res.contents

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dt)

        offset = np.ctypeslib.as_array(r.offset, shape=(k + 1,)).copy()
        out = IndexResult(accuracy, arr(r.header, k, np.uint8), arr(r.zero_bits, k, np.uint32), offset,
                          arr(r.tables, int(offset[k]), np.uint8))
    finally:
        lib.ugpu_index_free(res)
    del bufs
    return out


def _host_decoded(data):
    """index_inputs' bytes of one input, in host memory: behind a UTF-8 BOM, or
    converted on the device when a UTF-16/32 BOM says so."""
    _, n, keep = _buffer_ptr(data)
    host = keep if isinstance(keep, np.ndarray) else keep.reshape(-1).cpu().numpy().view(np.uint8)
    enc, skip = detect_bom(host[:4].tobytes() if n else b"", n)
    if enc in (_lib.ENC_PLAIN, _lib.ENC_UTF8):
        return host[skip:]
    dev, m = decode_input(host)
    return dev[:m].cpu().numpy()


def index_inputs(inputs, accuracy=4, ignore_binary=False):
    """index_batch over the bytes reflex::Input delivers for each input: a UTF-8
    BOM is dropped, UTF-16/32 with a BOM is converted (detect_bom,
    decode_input)."""
    return index_batch([_host_decoded(d) for d in inputs], accuracy, ignore_binary)


def write_index_store(names, result, accuracy=None):
    """The bytes of a ._UG#_Store (src/ugrep-indexer.cpp:1725-1745): the magic,
    then per input the accuracy digit, the header byte, the length of the name
    (16 bits, little endian), the name and the table.  `result` is an
    IndexResult or a sequence of (header, table) pairs; names are str (encoded
    as the file system does) or bytes."""
    import os
    if isinstance(result, IndexResult):
        accuracy = result.accuracy if accuracy is None else accuracy
        result = [(int(result.header[i]), result.table(i)) for i in range(len(result))]
    if accuracy is None or not 0 <= accuracy <= 9:
        raise ValueError("accuracy is 0..9")
    if len(names) != len(result):
        raise ValueError("one name per record")
    out = [INDEX_MAGIC]
    for name, (header, table) in zip(names, result):
        name = (name if isinstance(name, bytes) else os.fsencode(name))[:65535]
        size = (1 << (header & 0x1F)) if header & 0x1F else 0
        if len(table) != size:
            raise ValueError("table of %d bytes under header 0x%02x" % (len(table), header))
        out += [bytes([0x30 + accuracy, header, len(name) & 0xFF, len(name) >> 8]), name, bytes(table)]
    return b"".join(out)


def parse_index_store(blob):
    """The records of a ._UG#_Store: [(name bytes, accuracy, header, table bytes)]."""
    blob = bytes(blob)
    if blob[:5] != INDEX_MAGIC:
        raise ValueError("not an index store")
    out, p = [], 5
    while p < len(blob):
        if p + 4 > len(blob):
            raise ValueError("truncated record")
        acc, header = blob[p] - 0x30, blob[p + 1]
        ln = blob[p + 2] | (blob[p + 3] << 8)
        size = (1 << (header & 0x1F)) if header & 0x1F else 0
        q = p + 4 + ln + size
        if q > len(blob):
            raise ValueError("truncated record")
        out.append((blob[p + 4:p + 4 + ln], acc, header, blob[p + 4 + ln:q]))
        p = q
    return out


def index_directory(path, accuracy=4, ignore_binary=False):
    """Indexes the regular, non-hidden files of one directory (symbolic links
    are skipped) and writes its ._UG#_Store, names in sorted order; returns
    (names, IndexResult).  No recursion, archives, ignore files or incremental
    update."""
    import os
    names = sorted(e.name for e in os.scandir(path)
                   if not e.name.startswith(".") and e.is_file(follow_symlinks=False) and not e.is_symlink())
    datas = []
    for nm in names:
        with open(os.path.join(path, nm), "rb") as f:
            datas.append(f.read())
    res = index_inputs(datas, accuracy, ignore_binary)
    with open(os.path.join(path, INDEX_STORE), "wb") as f:
        f.write(write_index_store(names, res))
    return names, res


# --- the index query: which records of an index may match a pattern ---

_DEVICES = []


def _device_visible():
    if not _DEVICES:
        n = ctypes.c_int()
        _DEVICES.append(lib.ugpu_device_count(ctypes.byref(n)) == _lib.UGPU_OK and n.value > 0)
    return _DEVICES[0]


class IndexQuery:
    """The hash finite automaton of a pattern (ugpu_hfa_create, what ugrep
    --index builds with Pattern option h) and its query over index tables.
    Unsupported is raised for a pattern the native compiler refuses: keep every
    file then.  `words`: a flattened automaton (ugpu_hfa_import) in place of a
    pattern."""

    def __init__(self, pattern=None, fixed=False, icase=False, words=None):
        h = ctypes.c_void_p()
        if words is not None:
            w = np.ascontiguousarray(words, dtype=np.uint32)
            check(lib.ugpu_hfa_import(w.ctypes.data_as(_lib.c_u32p), w.size, ctypes.byref(h)))
        else:
            rx = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
            check(lib.ugpu_hfa_create(rx, len(rx), (RX_FIXED if fixed else 0) | (RX_ICASE if icase else 0),
                                      ctypes.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    @property
    def info(self):
        """dict of ugpu_hfa_info: has_hfa, levels, states, entries, ranges, truncated, hashes."""
        i = _lib.HfaInfo()
        check(lib.ugpu_hfa_info(self._h, ctypes.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in _lib.HfaInfo._fields_}

    def words(self):
        """The flattened automaton (ugpu_hfa_export; empty: no automaton)."""
        n = ctypes.c_uint64()
        check(lib.ugpu_hfa_export(self._h, None, 0, ctypes.byref(n)))
        w = np.zeros(max(n.value, 1), np.uint32)
        check(lib.ugpu_hfa_export(self._h, w.ctypes.data_as(_lib.c_u32p), w.size, ctypes.byref(n)))
        return w[:n.value]

    def match_host(self, table):
        """ugpu_hfa_match_host: whether a file with this index table may match."""
        t = np.frombuffer(bytes(table), np.uint8) if not isinstance(table, np.ndarray) else np.ascontiguousarray(table)
        keep = ctypes.c_int()
        check(lib.ugpu_hfa_match_host(self._h, t.ctypes.data_as(_lib.c_u8p), t.size, ctypes.byref(keep)))
        return bool(keep.value)

    def keep_host(self, header, table, ignore_binary=False, decompress=False):
        """The decision for one record on the host (src/ugrep.cpp:10060-10099)."""
        if not self.info["has_hfa"]:
            return True  # the index is off for such a pattern, whatever the header says (src/ugrep.cpp:8931)
        if (header & 0x80 and ignore_binary) or (header & 0x60 and not decompress):
            return False
        return self.match_host(table) if header & 0x1F else bool(header & 0x80)

    def query(self, result_or_tables, ignore_binary=False, decompress=False, force=None, device=None):
        """One keep flag (numpy bool) per record of an IndexResult, of
        parse_index_store's output (a list of (name, accuracy, header, table)),
        both through ugpu_index_query_records, or of the device form (d_tables,
        header, offset) as index_tables leaves it (ugpu_index_query).  force:
        "lds" or "global" pins where the kernel reads the tables.  device:
        False runs the host evaluator (ugpu_hfa_query_host) over host tables,
        which is also what None does when no device is visible."""
        flags = ((_lib.QUERY_IGNORE_BINARY if ignore_binary else 0) | (_lib.QUERY_DECOMPRESS if decompress else 0) |
                 {None: 0, "lds": _lib.QUERY_FORCE_LDS, "global": _lib.QUERY_FORCE_GLOBAL}[force])
        r = result_or_tables
        on_host = isinstance(r, (IndexResult, list))
        if isinstance(r, IndexResult):
            tables, header, offset = r.tables, r.header, r.offset
        elif isinstance(r, list):
            header = np.array([h for _, _, h, _ in r], dtype=np.uint8)
            offset = np.concatenate([[0], np.cumsum([len(t) for _, _, _, t in r])]).astype(np.uint64)
            tables = np.frombuffer(b"".join(bytes(t) for _, _, _, t in r), np.uint8)
        else:
            tables, header, offset = r
        header = np.ascontiguousarray(header, dtype=np.uint8)
        offset = np.ascontiguousarray(offset, dtype=np.uint64)
        n = header.size
        if offset.size != n + 1:
            raise ValueError("offset holds one value per record and the tables' length")
        keep = np.zeros(n + 1, np.uint8)
        hp, op, kp = header.ctypes.data_as(_lib.c_u8p), offset.ctypes.data_as(_lib.c_u64p), keep.ctypes.data_as(_lib.c_u8p)
        if on_host:
            tables = np.ascontiguousarray(tables, dtype=np.uint8)
            if device is None:
                device = _device_visible()
            fn = lib.ugpu_index_query_records if device else lib.ugpu_hfa_query_host
            check(fn(self._h, tables.ctypes.data_as(_lib.c_u8p), hp, op, n, flags, kp))
        else:
            check(lib.ugpu_index_query(self._h, ctypes.c_void_p(tables or None), hp, op, n, flags, kp, None))
        return keep[:n].astype(bool)

    @staticmethod
    def kernel_ms():
        """ugpu_index_query_kernel_ms: the device time of this thread's last query."""
        ms = ctypes.c_float()
        check(lib.ugpu_index_query_kernel_ms(ctypes.byref(ms)))
        return ms.value

    def _query_store(self, blobs, flags):
        """(keep, [(blob index, name bytes)]) over store blobs."""
        blobs = [bytes(b) for b in blobs]
        k = len(blobs)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in blobs])
        lens = np.array([len(b) for b in blobs], dtype=np.uint64)
        res = ctypes.POINTER(_lib.QueryResult)()
        check(lib.ugpu_index_query_store(self._h, ptrs, lens.ctypes.data_as(_lib.c_u64p), k, flags, ctypes.byref(res)))
        try:
            r = res.contents
            n = r.nrec
            keep = np.ctypeslib.as_array(r.keep, shape=(n,)).astype(bool) if n else np.zeros(0, bool)
            names = [(int(r.name_blob[i]), blobs[r.name_blob[i]][r.name_off[i]:r.name_off[i] + r.name_len[i]])
                     for i in range(n)]
        finally:
            lib.ugpu_query_free(res)
        return keep, names

    def close(self):
        if self._h:
            lib.ugpu_hfa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def query_index_store(path_or_blob, pattern, fixed=False, icase=False, ignore_binary=False, decompress=False):
    """ugpu_index_query_store over one ._UG#_Store (a path, or its bytes):
    (names, keep), the records' names as bytes in the store's order and one
    bool each.  A pattern the native compiler refuses keeps every record."""
    if isinstance(path_or_blob, (bytes, bytearray, memoryview)):
        blob = bytes(path_or_blob)
    else:
        with open(path_or_blob, "rb") as f:
            blob = f.read()
    flags = (_lib.QUERY_IGNORE_BINARY if ignore_binary else 0) | (_lib.QUERY_DECOMPRESS if decompress else 0)
    try:
        q = pattern if isinstance(pattern, IndexQuery) else IndexQuery(pattern, fixed, icase)
    except _lib.Unsupported:
        names = [p[0] for p in parse_index_store(blob)]
        return names, np.ones(len(names), bool)
    keep, names = q._query_store([blob], flags)
    return [nm for _, nm in names], keep


def find_indexed(pattern, inputs, index=None, fixed=False, icase=False, accuracy=4, offsets=True):
    """Index, query, scan the survivors: find_batch(Pattern(compile_regex(
    pattern)), inputs) computed over only the inputs whose index record may
    match.  index: an IndexResult of the inputs (index_batch is run when None).
    Returns a BatchResult equal to find_batch's over all inputs (a skipped
    input has no match, so its records are none), with .kept, one bool per
    input: whether it was scanned.  The inputs are host memory, as for
    find_batch.  A skipped input is neither packed, uploaded nor scanned; its
    bytes are still read once on the host to count its newlines, only so that
    .newlines equals find_batch's."""
    inputs = list(inputs)
    if index is None:
        index = index_batch(inputs, accuracy)
    if len(index) != len(inputs):
        raise ValueError("one index record per input")
    try:
        keep = IndexQuery(pattern, fixed, icase).query(index)
    except _lib.Unsupported:
        keep = np.ones(len(inputs), bool)
    pat = Pattern(compile_regex(pattern, fixed, icase))
    kept = [i for i in range(len(inputs)) if keep[i]]
    sub = find_batch(pat, [inputs[i] for i in kept], offsets)
    k = len(inputs)
    count = np.zeros(k, np.uint64)
    digest, dcap = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
    newlines, mlines = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
    for i in range(k):
        if not keep[i]:
            _, n, hold = _buffer_ptr(inputs[i])
            if not isinstance(hold, np.ndarray):
                if hold.is_cuda:
                    raise TypeError("find_indexed takes host inputs, as find_batch does")
                hold = hold.reshape(-1).numpy().view(np.uint8)
            newlines[i] = np.count_nonzero(hold[:n] == 10)
    for j, i in enumerate(kept):
        count[i] = sub.first[j + 1] - sub.first[j]
        digest[i], dcap[i], newlines[i], mlines[i] = sub.digest[j], sub.dcap[j], sub.newlines[j], sub.matching_lines[j]
    first = np.concatenate([[0], np.cumsum(count)]).astype(np.uint64)
    out = BatchResult(sub.one_scan, sub.count, first, digest, dcap, newlines, mlines)
    if offsets:  # (the kept inputs' records are already in input order)
        out.start, out.length, out.cap, out.line = sub.start, sub.length, sub.cap, sub.line
    out.kept = keep
    return out
