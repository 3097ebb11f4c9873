/*
 * ugpu.h -- C ABI of the MI355X DFA buffer-scan engine (ugrep_amd).
 *
 * This is the drop-in boundary for ugrep's hot path: the FIND loop of
 * reflex::Matcher::match(Const::FIND) (reference lib/matcher.cpp:42-750), i.e.
 * the adv_ prefilters (lib/matcher.cpp:797-954, lib/matcher_avx2.cpp:78-799,
 * lib/matcher_avx512bw.cpp:50-463) plus the DFA opcode walk (lib/matcher.cpp:
 * 125-546), driven by `while (matcher->find())` (src/ugrep.cpp:10544, :10869).
 *
 * Input artifact: the reference's compiled pattern, Pattern::opc_[0..nop_)
 * (include/reflex/pattern.h:1302-1304; word format :1155-1247; produced by
 * Pattern::encode_dfa, lib/pattern.cpp:2823-3063).  The same words are what the
 * reference's precompiled-table constructor Pattern(const Opcode*, ...) takes
 * (include/reflex/pattern.h:151-159), so a caller passes pattern.opc_ as is.
 *
 * Semantics: identical match records (start, length, accept index) to
 * Matcher::find() on a fully buffered input (AbstractMatcher::buffer(),
 * include/reflex/absmatcher.h:542-591): leftmost-longest, non-overlapping,
 * empty matches rejected unless option N (UGPU_PAT_EMPTY), option A off;
 * option W by UGPU_PAT_WORD.  Line anchors (META_BOL/META_EOL) and word
 * boundaries (META_WBB/WBE/WEB/WEE/NWB/NWE/BWB/EWB) at the start or end of a
 * match become per-context accepts.  Tables with
 * lookahead HEAD/TAIL words, buffer anchors (META_BOB/EOB), assertions between
 * consumed characters, or REDO words return UGPU_UNSUPPORTED; the caller keeps
 * its CPU matcher for those (include/reflex/pattern.h:1194-1217).
 *
 * All functions return an int status; no exceptions cross this ABI (reference
 * errors: regex_error lib/pattern.cpp:162-169, std::bad_alloc absmatcher.h:401).
 * Handles are opaque.  A ugpu_dfa is immutable after creation and may be shared
 * by threads (the reference shares one Pattern across GrepWorker clones,
 * src/ugrep.cpp:4146-4149, :4206); a ugpu_scanner is per thread/stream.
 */
#ifndef UGPU_H
#define UGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define UGPU_OK 0
#define UGPU_UNSUPPORTED 1 /* table needs lookahead/REDO/inner assertions: use the CPU matcher */
#define UGPU_INVAL 2       /* bad argument or malformed opcode table */
#define UGPU_NOMEM 3       /* host or device allocation failed */
#define UGPU_DEVICE 4      /* HIP runtime error (see ugpu_last_error) */
#define UGPU_HALO 5        /* a match walked past readable bytes of a non-final shard */
#define UGPU_CAPACITY 6    /* more matches than the caller's output capacity */

/* scan modes */
#define UGPU_MODE_COUNT 0   /* count + digests only */
#define UGPU_MODE_OFFSETS 1 /* also materialize (start, len, cap) records */

/* ABI version of this header: bumped whenever a struct below changes layout
   or an entry point is added (ugpu_dfa_info gained contexts/shape in ABI 2;
   ugpu_stream_reserve came in ABI 3).  A caller compiled against
   one header checks ugpu_abi_version() == UGPU_ABI_VERSION before passing a
   struct to the library (integration/reflex_gpu_matcher.h does; on a mismatch
   it keeps the CPU matcher). */
#define UGPU_ABI_VERSION 3

typedef struct ugpu_dfa ugpu_dfa;
typedef struct ugpu_scanner ugpu_scanner;

typedef struct ugpu_dfa_info
{
  uint32_t states;      /* DFA states including the dead state */
  uint32_t classes;     /* byte equivalence classes */
  uint32_t row;         /* table row width (256 = byte-indexed, else class-indexed, pow2) */
  uint32_t format;      /* 0 = next[state][byte], 1 = cls[byte] + next[state][class] */
  uint32_t table_bytes; /* bytes of the transition table staged in LDS */
  uint32_t prefilter_ppm; /* prefiltered (sparse) scan: est. candidate positions per million + 1; 0 = dense scan */
  uint32_t first_bytes; /* number of bytes that can start a match (|fst_|) */
  uint32_t accepting;   /* accepting states */
  uint32_t kernel;      /* kernel of a COUNT scan: 0 sparse (prefiltered), 1 dense, 2 xi (immediate
                           transducer; UGPU_XI=0 selects dense), 3 xg (gap transducer; UGPU_XG=0),
                           4 wfind (option W, UGPU_PAT_WORD), 5 xc (two-state carry chain; UGPU_XC=0),
                           6 xc U mode (code-point runs without a gap transducer; UGPU_XU=1 prefers it,
                           UGPU_XU=0 never), 7 ngram (class and wide tables behind an n-gram candidate
                           filter, e.g. large string sets; UGPU_NG=0 restores kernel 1 / 4; then
                           prefilter_ppm is the filter's estimate) */
  uint32_t contexts;   /* accept contexts per state of the per-context accepts (ugpu_tables_context_host):
                           1 = none (no meta edges), 4 = line anchors (bol * 2 + eol), 64 = word boundaries
                           (ugrep_amd/csrc/ctx_bits.hpp) */
  uint32_t shape;       /* UGPU_SHAPE_* bits (the drop-in matcher's test of where the reference's
                           match predictor is exact for word-boundary patterns) */
} ugpu_dfa_info;

#define UGPU_SHAPE_FINITE 1u     /* the language is finite (no cycle in the DFA) */
#define UGPU_SHAPE_WORD_COND 2u  /* a state whose accept depends on a word boundary also has byte edges */
#define UGPU_SHAPE_ONE_ACCEPT 4u /* every match has the same accept index: 12-byte records (ugpu_scan_offsets d_cap NULL) */
#define UGPU_SHAPE_LOOKAHEAD 16u /* lookahead (X(?=Y): TAIL/HEAD words): the lookahead walk on wfind_kernel */
#define UGPU_SHAPE_LOOP_NEEDLE 8u /* C+ N on the sparse kernel: the prefilter looks for the needle N and walks back
                                     (UGPU_LB=0 disables) */
#define UGPU_SHAPE_FILTER2 32u /* the sparse kernel's prefilter tests two of a byte's three bit fields: it adds few
                                  candidates for this table (UGPU_FT2=0 / 1 forces it) */
#define UGPU_SHAPE_NGRAM 64u /* the table scans behind the n-gram candidate filter (kernel 7; UGPU_NG=0 disables;
                                DESIGN.md 3.1a) */

/* Totals of one scan.  digest = sum(start*31 + len), dcap = sum((start+1)*cap),
   both mod 2^64, start = byte offset + bias. */
typedef struct ugpu_totals
{
  uint64_t count;
  uint64_t digest;
  uint64_t dcap;
  uint64_t entry;  /* chain position entering the range (== lo for a fresh scan) */
  uint64_t exit;   /* first chain position >= hi: where the search resumes after the range */
  uint32_t flags;  /* bit0: a walk hit the readable end of a non-final shard (UGPU_HALO);
                      bit3 (UGPU_TOT_FOREST): the speculative stitch did not converge (FIND chains
                      that never resynchronise, e.g. \D\D over text without digits) and the range
                      was resolved exactly by the forest FIND (ugrep_amd/csrc/forest.hip);
                      bit4 (UGPU_TOT_WFAST): option W on a \w+ table ran the non-W kernels
                      (the scanned bytes are valid UTF-8, so W removes nothing) */
  uint32_t fix_rounds;
} ugpu_totals;

#define UGPU_TOT_FOREST 8u
#define UGPU_TOT_WFAST 16u

/* Library-owned match list for ugpu_find_all. */
typedef struct ugpu_result
{
  uint64_t count;
  uint64_t digest;
  uint64_t dcap;
  uint64_t *start; /* count entries, byte offsets relative to buf */
  uint32_t *len;
  uint32_t *cap;   /* accept index (Matcher::accept(), absmatcher.h:605-609) */
} ugpu_result;

/* --- pattern tables (replaces the Pattern -> Matcher table consumer) --- */

/* Build the dense device tables from opcode words and upload them once to the
   current device.  pattern_flags: 0, or UGPU_PAT_WORD for Matcher option W
   (ugrep -w: matches bounded by word boundaries, src/ugrep.cpp:8616-8618,
   lib/matcher.cpp:107, :142, :208, include/reflex/matcher.h:1194-1237); at_wb
   at a walk start reads the code point before it, so dbuf[0] counts as the
   begin of the input and a scan that starts inside the input passes the bytes
   before lo in dbuf (4 suffice; ugpu_find_all_multi and the stream API do).
   UGPU_PAT_EMPTY: Matcher option N (ugrep -Y, and -x:
   src/ugrep.cpp:8381-8386, :8612-8613), empty matches are reported
   (lib/matcher.cpp:682-728; never at the end of the input).  Tables with line
   anchors (META_BOL ^, META_EOL $ edges, include/reflex/pattern.h:942-943, as
   ugrep -x makes, src/cnf.hpp:167-185) are accepted; other meta edges (word
   boundaries, \A, \Z, indent) return UGPU_UNSUPPORTED.  Anchored tables, and
   tables that match the empty string under option N, scan on the exact context
   walk (wfind_kernel; its W rules replaced by the anchor rules): bol at a walk
   start is "the byte before is '\n' or the position is the buffer begin"
   (see ugpu_scanner_context for buffers that do not begin the input), eol is
   "the next byte is '\n', EOF, or '\r' before '\n'".  W together with anchors
   or empty matches returns UGPU_UNSUPPORTED. */
#define UGPU_PAT_WORD 1u
#define UGPU_PAT_EMPTY 2u
int ugpu_dfa_create(const uint32_t *opc, uint32_t nop, uint32_t pattern_flags, ugpu_dfa **out);
/* Releases made once the process is exiting (exit() or a return from main:
   static destructors, atexit handlers that run after the engine's own) free
   nothing and return UGPU_OK -- the HIP runtime may already be torn down --
   for ugpu_dfa_destroy, ugpu_scanner_destroy, ugpu_stream_destroy and
   ugpu_records_free; ugpu_select_device makes no HIP call then. */
int ugpu_dfa_destroy(ugpu_dfa *dfa);
int ugpu_dfa_info_get(const ugpu_dfa *dfa, ugpu_dfa_info *info);

/* Host-only: what ugpu_dfa_create(opc, nop, pattern_flags) would return
   (UGPU_OK, UGPU_UNSUPPORTED, UGPU_INVAL) and, on UGPU_OK, the info it would
   report (the kernel a COUNT scan runs) -- without touching a device, so a
   caller can decide whether a device is worth initialising (the drop-in
   matcher decides CPU or GPU per input before any HIP call). */
int ugpu_dfa_plan_host(const uint32_t *opc, uint32_t nop, uint32_t pattern_flags, ugpu_dfa_info *info);

/* Host-only: build the dense tables without touching a device (inspection and
   CPU tests).  trans gets states*row u16 entries (entry = target_state*row,
   0 = dead), cls 256 bytes, caps `states` accept indices; *start is the start
   entry, *accb the first accepting entry.  Pass NULL arrays to query sizes
   through info first. */
int ugpu_tables_build_host(const uint32_t *opc, uint32_t nop, ugpu_dfa_info *info, uint16_t *trans,
                           uint32_t trans_cap, uint8_t *cls, uint32_t *caps, uint32_t caps_cap, uint32_t *start,
                           uint32_t *accb);

/* Host-only: the prefilter lookup tables (T0[8], T1[8], T2[4] bucket bytes, see
   ugrep_amd/csrc/tables.hpp) into ft[20]; returns UGPU_OK and sets *enabled to 1
   when the sparse (prefiltered) kernel is used for this table. */
int ugpu_tables_prefilter_host(const uint32_t *opc, uint32_t nop, uint8_t *ft, int *enabled);

/* Host-only: the FIND transducer table of a restart-local DFA (see
   ugrep_amd/csrc/tables.hpp: entries = row | XT_DEAD(1) | XT_LIVE(2)), same
   shape as trans.  *local = 0 (and nothing written) when the table is not
   restart-local; then the dense kernel uses its general walk. */
int ugpu_tables_transducer_host(const uint32_t *opc, uint32_t nop, uint16_t *xtrans, uint32_t xtrans_cap,
                                int *local);

/* Host-only: the immediate FIND transducer of xi_kernel (ugrep_amd/csrc/
   tables.hpp): for restart-local tables whose walks accept on every byte,
   u8 ids (walk state << 3 | SYNC 4 | IN 2 | START 1), rows*256 bytes of
   next ids.  *immediate = 0 (nothing written) when the table does not qualify;
   pass xid = NULL to query *rows first. */
int ugpu_tables_immediate_host(const uint32_t *opc, uint32_t nop, uint8_t *xid, uint32_t xid_cap, uint32_t *rows,
                               uint8_t *sync_byte, int *immediate);

/* Host-only: the gap transducer of xg_kernel (ugrep_amd/csrc/tables.hpp):
   xtrans entries plus XG_A (4, the new state accepts) and the accept's
   gap + 1 in bits 3-5, same shape as trans; sync[256] = sync-byte flags.
   *gap = 0 (nothing written) when the table does not qualify. */
int ugpu_tables_gap_host(const uint32_t *opc, uint32_t nop, uint16_t *xg, uint32_t xg_cap, uint8_t *sync, int *gap);

/* Host-only: the byte classes of xc_kernel (two-state tables: start --G--> A
   --X--> A, ugrep_amd/csrc/tables.hpp): cls[256] = G << 7 | X << 6 (may be
   NULL).  *ok = 0 when the table does not qualify.  (Replaces, for these
   tables, the per-byte opcode scan of lib/matcher.cpp:460-545.) */
int ugpu_tables_xc_host(const uint32_t *opc, uint32_t nop, uint8_t *cls, int *ok);

/* Host-only: the code-point run tables of a table whose language is S+ for a
   set S of single-code-point tokens (\w+, \S+, [[:alpha:]]+ over UTF-8;
   ugrep_amd/csrc/tables.hpp xu_*): tab[256 + 64 * 256 + 256] token codes and
   bm3[2048] third-byte bits (either may be NULL).  *ok = 0 when the table does
   not qualify.  (Replaces, for these tables, the per-byte opcode scan of
   lib/matcher.cpp:460-545.) */
int ugpu_tables_xu_host(const uint32_t *opc, uint32_t nop, uint8_t *tab, uint32_t *bm3, int *ok);

/* Host-only: the dominated-restart bits of the dense tables (bit s of
   dom[s / 32], state numbering as ugpu_tables_build_host): L(start) is a
   subset of L(s), so a failed FIND walk that crosses position q in state s
   shows that no match starts at q (the chain skips it; ugrep_amd/csrc/
   tables.hpp dom).  *n = the number of u32 words (0: not computed, no skips);
   *all (may be NULL) = 1 when every non-accepting state reachable from the
   start has its bit (then a failed walk skips up to the byte it died on).
   (Replaces the reference's position-by-position restart after a failed
   match, lib/matcher.cpp:692-713, for the stitching re-walks.) */
int ugpu_tables_dom_host(const uint32_t *opc, uint32_t nop, uint32_t *dom, uint32_t dom_cap, uint32_t *n, int *all);

/* Host-only: the n-gram candidate filter of kernel 7 (ugrep_amd/csrc/ngram.hpp,
   tables.hpp ng_*) under pattern_flags (UGPU_PAT_*): *n = the n-gram length
   (2-4; 0: the table has none), *log2_bits = log2 of the bitmap's bits, bitmap
   = its 2^log2_bits / 32 u32 words (NULL: size query; bitmap_cap in words),
   *ppm = the estimated candidate positions per million on text, *enabled = 1
   when the plan takes kernel 7 for this table.  Bit ngram_hash(window) is set
   for every n-byte string that begins a match, so every match start tests
   positive.  (Replaces the reference's PM4 predictor and advance_pattern_pma,
   include/reflex/pattern.h:389-401, lib/matcher.cpp:2465-2489.) */
int ugpu_tables_ngram_host(const uint32_t *opc, uint32_t nop, uint32_t pattern_flags, uint32_t *n,
                           uint32_t *log2_bits, uint32_t *bitmap, uint32_t bitmap_cap, uint32_t *ppm, int *enabled);

/* Host-only: flags_out[p] = 1 where the n-gram filter, as the device evaluates
   it over the whole buffer buf[0, len) (the end of the input), makes position
   p a candidate: p + n <= len and its window tests positive; else 0.  Fails
   with UGPU_UNSUPPORTED for a table without an n-gram filter.  (The test form
   of the predictor loop, lib/matcher.cpp:2465-2489.) */
int ugpu_ngram_candidates_host(const uint32_t *opc, uint32_t nop, uint32_t pattern_flags, const uint8_t *buf,
                               uint64_t len, uint8_t *flags_out);

/* Host-only: the per-context accept indices of the dense tables (states * 4
   u32: acap[state * 4 + bol * 2 + eol], state numbering as
   ugpu_tables_build_host), whether the table has line anchors, and whether its
   start state accepts in some context (empty matches). */
int ugpu_tables_context_host(const uint32_t *opc, uint32_t nop, uint32_t *acap, uint32_t acap_cap, int *anchored,
                             int *start_acc);

/* Host-only: *eq = 1 when two opcode tables accept the same strings with the
   same accept indices (so their FIND chains agree on every input).  The
   engine uses it to recognise \w+ under option W. */
int ugpu_tables_equivalent_host(const uint32_t *opc_a, uint32_t nop_a, const uint32_t *opc_b, uint32_t nop_b, int *eq);

/* --- whole-buffer FIND (Matcher::buffer(); while (find()) ...) --- */

/* buf may be host or device memory, len bytes, search starts at `start`
   (the matcher's cur_).  Synchronous.  mode: UGPU_MODE_COUNT or _OFFSETS. */
int ugpu_find_all(const ugpu_dfa *dfa, const uint8_t *buf, uint64_t len, uint64_t start, uint32_t mode,
                  ugpu_result **out);
int ugpu_result_free(ugpu_result *res);

/* Records for a consumer that pops them one at a time (the drop-in matcher's
   find() loop, lib/matcher.cpp:42-750 returning one match per call), at the
   rate PCIe moves the input: a host buffer goes H2D in chunks
   (UGPU_REC_CHUNK, default 64 MiB) on a copy thread, each chunk is scanned
   from the true chain entry as soon as it (and a 1 MiB halo) is resident, its
   records are packed to 6 B (8 B when the table has several accept indices)
   and copied asynchronously into pinned host memory, so input copy, scans and
   record copy overlap.  ugpu_find_records returns once the last input byte is
   on the device (a host buffer may then go away); scans and record copies go
   on behind the consumer on a pipeline thread.  ugpu_records_next pops the
   records in chain order, waiting for the pipeline where needed (1 = a record,
   0 = none left, -code on a pipeline error, after which the consumer may go on
   from the last record's end on the CPU: FIND chains agree there; start, len
   and cap must not be NULL); ugpu_records_totals waits for the end and equals
   ugpu_find_all's totals.  A device buffer must stay valid until
   ugpu_records_free, which waits for the pipeline. */
typedef struct ugpu_records ugpu_records;
int ugpu_find_records(const ugpu_dfa *dfa, const uint8_t *buf, uint64_t len, uint64_t start, ugpu_records **out);
/* ugpu_find_records with flags.  UGPU_REC_BORROW: the caller keeps buf
   readable until ugpu_records_free returns (which stops and joins the
   pipeline), so the call returns at once and the first records can be popped
   while the rest of the input is still crossing PCIe.  Plain
   ugpu_find_records returns only once the last input byte is on the device
   (ugrep may unmap a file as soon as it stops asking for matches). */
#define UGPU_REC_BORROW 1u
int ugpu_find_records_ex(const ugpu_dfa *dfa, const uint8_t *buf, uint64_t len, uint64_t start, uint32_t flags,
                         ugpu_records **out);
int ugpu_records_next(ugpu_records *r, uint64_t *start, uint32_t *len, uint32_t *cap);
int ugpu_records_totals(ugpu_records *r, uint64_t *count, uint64_t *digest, uint64_t *dcap);
/* Pop every remaining record, returning their number and digests (what a
   native consumer's loop costs; tests and benchmarks). */
int ugpu_records_drain(ugpu_records *r, uint64_t *n, uint64_t *digest, uint64_t *dcap);
int ugpu_records_free(ugpu_records *r);

/* Multi-device FIND (the reference has no counterpart: one
   buffer is always scanned by one thread, src/ugrep.cpp:4118-4480).  One
   process drives the devices: [start, len) is cut into `ndev` contiguous
   shards at arbitrary byte offsets; shard k runs on device k mod
   hipGetDeviceCount() (so ndev may exceed the devices: virtual shards share a
   card), each with its own table copy, its own input copy (host buffers: H2D
   over that device's PCIe link; a device buffer: a peer copy over xGMI for
   the shards on other devices) plus a 1 MiB halo, and its own stream.  The
   shards' FIND chains are then resolved left to right on the host
   (ugpu_chain_fix on the owning device when a chain enters a shard elsewhere
   than at its start), and OFFSETS records are copied straight from each
   device into their slice of the result.  Same result as ugpu_find_all.
   Each shard's copy starts 4 bytes before it (the code point at_wb reads for
   option W, the byte at_bol reads for line anchors).  ndev <= 0: one shard per
   device. */
int ugpu_find_all_multi(const ugpu_dfa *dfa, const uint8_t *buf, uint64_t len, uint64_t start, uint32_t mode,
                        int ndev, ugpu_result **out);

/* --- device-resident scanning (benchmarks, multi-GPU shards) --- */

/* Workspace for scans of device buffers on the current device. */
int ugpu_scanner_create(const ugpu_dfa *dfa, ugpu_scanner **out);
/* UGPU_SCANNER_RECORDS: the scans will be followed by ugpu_scan_offsets --
   prefer kernels with their own record-writing pass (code-point run tables
   take xc_kernel's U mode instead of xg_kernel, whose OFFSETS are rebuilt on
   dense_kernel).  Results never depend on it. */
#define UGPU_SCANNER_RECORDS 1u
int ugpu_scanner_create_ex(const ugpu_dfa *dfa, uint32_t flags, ugpu_scanner **out);
int ugpu_scanner_destroy(ugpu_scanner *sc);

/* Enqueue a COUNT scan of dbuf[lo..hi) on `stream` (hipStream_t, NULL = default).
   Walks may read up to read_end; at_eof says read_end is the end of the whole
   stream.  Reported starts are offset by `bias` (global shard offset).
   Asynchronous: results are read with ugpu_scan_totals. */
int ugpu_scan(ugpu_scanner *sc, const uint8_t *dbuf, uint64_t lo, uint64_t hi, uint64_t read_end, int at_eof,
              uint64_t bias, void *stream);
/* Context of the scanner's next scans: bol0 != 0 when dbuf[0] begins a line
   (it is the first byte of the input, or the byte before it is '\n'); the
   default is 1.  Only line-anchored tables read it, for a walk at dbuf[0];
   walks after dbuf[0] read the byte before them (the library's own shards and
   streams keep 4 bytes before their range in dbuf instead). */
int ugpu_scanner_context(ugpu_scanner *sc, int bol0);
/* Synchronize the scanner's stream and return the totals of the last scan. */
int ugpu_scan_totals(ugpu_scanner *sc, ugpu_totals *out);
/* After ugpu_scan + ugpu_scan_totals: write the match records of the last scan
   into device arrays (capacity entries each) on `stream`.  d_cap may be NULL
   for a table with one accept index (ugpu_dfa_info.accepting states all take
   the same index; the records are then 12 bytes: start, len) -- the accept
   index of every record is that index; UGPU_INVAL for other tables.
   UGPU_UNSUPPORTED when a match of the scan is 2^32 bytes or longer (its
   length does not fit a record; the totals of the COUNT scan stay valid):
   no record of such a scan is to be used.  ugpu_find_all in OFFSETS mode and
   the other record-returning calls return the same. */
int ugpu_scan_offsets(ugpu_scanner *sc, uint64_t *d_start, uint32_t *d_len, uint32_t *d_cap, uint64_t capacity,
                      void *stream);
/* Shard-boundary stitch: the scan of [lo,hi) assumed the chain entered at
   old_entry; the true chain enters at new_entry.  Returns the correction to add
   to the totals and the (possibly changed) exit.  Synchronous. */
int ugpu_chain_fix(ugpu_scanner *sc, const uint8_t *dbuf, uint64_t lo, uint64_t hi, uint64_t read_end, int at_eof,
                   uint64_t bias, uint64_t old_entry, uint64_t new_entry, ugpu_totals *delta, void *stream);
/* Single-pass OFFSETS: with on != 0, COUNT scans of prefiltered tables also
   stage each wave's records, and ugpu_scan_offsets copies them to the output
   (plus a WRITE pass over the waves whose speculative chain was not the true
   one) instead of re-running the scan.  ugpu_find_all in OFFSETS mode does
   this by itself.  Costs 16 B of staging per record (128 MiB per scanner). */
int ugpu_scanner_stage(ugpu_scanner *sc, int on);
/* Time (ms) of the scan kernel of the last ugpu_scan, measured with HIP events
   recorded on the scan stream around that launch. */
int ugpu_scan_kernel_ms(ugpu_scanner *sc, float *ms);

/* --- streaming FIND ---
   Input fed in chunks (what AbstractMatcher::input() + grow()/peek_more()
   provide to Matcher::match, absmatcher.h:1417-1536, :1582-1593; ugrep streams
   stdin, decompressed data and files it does not mmap, src/ugrep.cpp:3936-3944).
   Each ugpu_stream_feed() scans the unsettled tail of the previous chunks plus
   the new chunk on the device and returns the matches that are final: the
   FIND chain is settled up to a point `keep` bytes before the end (or the end
   when `final`), the rest is carried to the next call.  Offsets are absolute
   (from the first byte ever fed); a match may span any number of chunks.  The
   concatenation of all results equals ugpu_find_all over the whole input
   (also for option W and line anchors: the carry keeps the 4 bytes before the
   settled position, the code point at_wb and the byte at_bol read). */
typedef struct ugpu_stream ugpu_stream;

/* keep: bytes held back from each non-final scan (a match that is still open
   that close to the end is re-scanned with the next chunk; 0 = 64 KiB). */
int ugpu_stream_create(const ugpu_dfa *dfa, uint64_t keep, ugpu_stream **out);
int ugpu_stream_destroy(ugpu_stream *st);

/* Feed host bytes; *out (free with ugpu_result_free) gets the newly final
   matches (records in OFFSETS mode) and their count/digest/dcap.
   final: 1 = the input ends with this chunk; UGPU_FEED_FLUSH = more input may
   follow, but settle every match the bytes so far decide (the input would
   block: a slow pipe or a TTY, whose reference matcher reports those matches
   before it waits, include/reflex/input.h:716-731); 0 = hold back `keep`. */
#define UGPU_FEED_FLUSH 2
int ugpu_stream_feed(ugpu_stream *st, const uint8_t *chunk, uint64_t len, int final, uint32_t mode,
                     ugpu_result **out);

/* Absolute offset up to which the FIND chain is settled (bytes before it will
   not be scanned again). */
uint64_t ugpu_stream_settled(const ugpu_stream *st);

/* Pre-create, on the calling thread's device, the pooled resources of `n`
   streams on this table whose feeds hold up to feed_bytes (scanners, device
   buffers and match lists, a private queue and a pinned block each), so that
   the streams created later allocate nothing (ugrep's workers otherwise make
   these device allocations all at once, and they serialise).  Optional: a
   stream without reserved resources creates them itself. */
int ugpu_stream_reserve(const ugpu_dfa *dfa, int n, uint64_t feed_bytes);

/* --- line-level consumers ---
   For a device-resident buffer (16-byte aligned; the kernels load whole
   16-byte granules, so the last granule is read up to its end and the bytes
   past len are ignored) and its sorted match starts
   (e.g. from ugpu_scan_offsets): *newlines = number of '\n' bytes in [0, len)
   (simd nlcount, lib/simd.cpp:62-166), d_line[i] = 1-based line of
   d_start[i] (AbstractMatcher::lineno(), absmatcher.h:695-766; d_line may be
   NULL), *matching_lines = number of distinct lines holding a match start
   (ugrep -c with skip('\n') after each hit, src/ugrep.cpp:10567-10586; equal
   to ugrep -c whenever matches cannot contain '\n').  Synchronous. */
int ugpu_lines(const uint8_t *dbuf, uint64_t len, const uint64_t *d_start, uint64_t n, uint64_t *d_line,
               uint64_t *newlines, uint64_t *matching_lines, void *stream);

/* Column, line begin and line of byte positions: the -k and -n of ugrep -onkb
   (-b is the position itself).  Same buffer rules as ugpu_lines.  d_pos is an
   ascending device list of n positions in [0, len] (repeats allowed), e.g. the
   match starts, or the ascending list of start + len for the match ends.  For
   a position p:
     d_bol[i]  = 1 + the offset of the last '\n' in [0, p), or 0 when there is
                 none (matcher->bol(); p - d_bol[i] is AbstractMatcher::border(),
                 absmatcher.h:1153-1157); a position on a '\n' belongs to the
                 line that newline ends, as in ugpu_select_lines;
     d_line[i] = 1 + the number of '\n' in [0, p): the d_line of ugpu_lines;
     d_col[i]  = AbstractMatcher::columno() (absmatcher.h:795-816), 0-based
                 (ugrep prints d_col + 1): the value of k after the fold over
                 the bytes [d_bol[i], p) from 0 in which a '\t' does
                 k += 1 + (~k & (tab - 1)) and any other byte
                 k += ((byte & 0xC0) != 0x80), so UTF-8 continuation bytes
                 count 0 and every other byte 1 ('\r', NUL and invalid UTF-8
                 included).
   tab is ugrep's --tabs=NUM (src/ugrep.cpp:6689-6691, default 8): 1, 2, 4 or
   8, anything else is UGPU_INVAL.  Each of the three arrays may be NULL, all
   three NULL is UGPU_INVAL (both are decided before the device is touched).
   A position > len gets UINT64_MAX in every output.  n == 0 and len == 0 are
   valid.  Synchronous. */
int ugpu_columns(const uint8_t *dbuf, uint64_t len, const uint64_t *d_pos, uint64_t n, uint32_t tab,
                 uint64_t *d_col, uint64_t *d_bol, uint64_t *d_line, void *stream);

/* --- line records (the bol/eol half) ---
   Same buffer rules as ugpu_lines.  Line k (1-based) is the bytes after the
   (k-1)-th '\n' up to and including the k-th; a non-empty tail after the last
   '\n' is a last, unterminated line; an empty buffer has no lines.  A line
   record is (begin, end, lineno): begin = offset of the line's first byte
   (matcher->bol()), end = offset of its '\n', or len for the unterminated
   line (matcher->eol(true) without the newline).

   ugpu_select_lines replaces the line loop of src/ugrep.cpp:11432-11521 for a
   sorted match list (d_len NULL: all lengths 0): a match (s, l) with s < len
   touches every line from the one holding byte s through the one holding byte
   min(max(s, s+l-1), len-1); a match starting on a '\n' belongs to the line
   that newline ends; matches with s >= len are ignored.  The touched lines
   (with UGPU_SEL_INVERT, ugrep -v: the untouched ones) are written once each,
   ascending, to d_begin/d_end/d_lineno (all three NULL: count only).
   *lines = number of lines, *selected = number of selected lines; when that
   exceeds capacity the call returns UGPU_CAPACITY with *selected valid and
   writes no record.  Synchronous. */
#define UGPU_SEL_INVERT 1u
int ugpu_select_lines(const uint8_t *dbuf, uint64_t len, const uint64_t *d_start, const uint32_t *d_len, uint64_t n,
                      uint32_t flags, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_lineno, uint64_t capacity,
                      uint64_t *selected, uint64_t *lines, void *stream);

/* (begin, end) of each line of an ascending device list of line numbers
   (repeats allowed), e.g. the context lines around a selection, a --range, or
   the d_line of ugpu_lines: matcher->bol() / eol(true) by line number.  Line 0
   or a line past the last gives UINT64_MAX in both fields.  Synchronous. */
int ugpu_line_spans(const uint8_t *dbuf, uint64_t len, const uint64_t *d_lineno, uint64_t n, uint64_t *d_begin,
                    uint64_t *d_end, void *stream);

/* --- Boolean line queries (ugrep --bool, -e A --and B --andnot C, --not, --files) ---
   ugpu_select_lines_bool replaces the per-line CNF check of the reference
   (cnf_matching, src/ugrep.cpp:3277-3376: one sub-matcher find() per literal
   over every candidate line; cnf_satisfied, :3379-3427, with --files) for a
   device-resident buffer that every sub-pattern has scanned once.

   Lines, line records and "a match touches a line" are those of
   ugpu_select_lines.  There are nlists <= UGPU_BOOL_MAX_LISTS sorted device
   match lists (d_starts[t], d_lens[t], n[t]); d_lens NULL or d_lens[t] NULL
   means all lengths of that list are 0; a list may be empty (n[t] == 0, its
   pointers may be NULL).  The pointer arrays d_starts, d_lens, n and clauses
   are host memory.  Literal t of a line is true when some match of list t
   touches the line.  A formula is nclauses <= UGPU_BOOL_MAX_CLAUSES clauses
   {pos, neg} over the literal bits of a line; a clause holds when
     (bits & pos) != 0 || (~bits & neg & listmask) != 0,  listmask = 2^nlists - 1,
   and the formula is the AND of its clauses (no clause: every line).  A mask
   bit at or above nlists, or a clause with pos == neg == 0, gives UGPU_INVAL.
   One clause {1, 0} over one list is ugpu_select_lines; {0, 1} is
   ugpu_select_lines with UGPU_SEL_INVERT.

   flags: UGPU_SEL_INVERT complements the selection per line.
   UGPU_BOOL_FILES (--files) evaluates the literals over the whole input
   (literal t is true when list t touches any line, i.e. has a match starting
   below len); when the formula then holds, the lines touched by any list are
   selected (the reference prints the lines of the adjoined pattern,
   CNF::adjoin, src/cnf.cpp:736-743), otherwise none; UGPU_SEL_INVERT
   complements that selection.  *whole (may be NULL) receives the formula's
   truth value over the whole-input literals; without UGPU_BOOL_FILES it
   receives whether any line is selected.

   Outputs and capacity as ugpu_select_lines: all three record arrays or none
   (count only); *selected and *lines are always valid; UGPU_CAPACITY with no
   record written when *selected > capacity; records ascending, once per line.

   The result is what ugrep --bool selects whenever no sub-pattern can match a
   '\n' (ugpu_tables_newline_host): then "list t touches the line" is
   "sub-matcher t finds something in [bol, eol]", and the reference's primary
   (adjoined) pattern never removes a line the CNF accepts: it is empty when
   every clause carries a NOT alternative (src/cnf.cpp:746-761).  For patterns
   that can match a newline the two differ, as matching_lines of ugpu_lines
   does.  Synchronous. */
#define UGPU_BOOL_FILES 2u
#define UGPU_BOOL_MAX_LISTS 16
#define UGPU_BOOL_MAX_CLAUSES 64
typedef struct ugpu_bool_clause { uint32_t pos, neg; } ugpu_bool_clause;
int ugpu_select_lines_bool(const uint8_t *dbuf, uint64_t len, const uint64_t *const *d_starts,
                           const uint32_t *const *d_lens, const uint64_t *n, uint32_t nlists,
                           const ugpu_bool_clause *clauses, uint32_t nclauses, uint32_t flags, uint64_t *d_begin,
                           uint64_t *d_end, uint64_t *d_lineno, uint64_t capacity, uint64_t *selected, uint64_t *lines,
                           int *whole, void *stream);

/* host-only: *nl = 1 when some match of the table can contain '\n', i.e. a
   state reachable from the start state has a live edge on byte 0x0a (anchors
   and word boundaries consume no byte and do not count). */
int ugpu_tables_newline_host(const uint32_t *opc, uint32_t nop, int *nl);

/* --- batched FIND: many inputs in one scan, with per-input records ---
   Replaces the per-file loop of the reference (src/ugrep.cpp:4261-4480, one
   job per file: each file gets its own matcher pass, its own line counter and
   its own totals) for inputs that are already in memory: the fixed cost of a
   FIND pass (an input copy, the launches, the host round trips, a result copy)
   is paid once per batch instead of once per file.

   The inputs are packed back to back into one buffer, each ended by '\n' (one
   is added to a non-empty input that lacks it; an empty input takes no bytes).
   When no match of the table can contain '\n', the FIND chain of the packed
   buffer passes through every input's first byte and its match list is the
   concatenation of the per-input lists: at_wb reads a preceding '\n' like the
   buffer begin, at_we and at_eol read a following '\n' like EOF, and bol after
   '\n' equals bol at the begin.  One exception: an input that
   ends in a bare '\r' -- at_eol is 0 for '\r' then EOF but 1 for "\r\n". */

/* Host-only: *one_scan = 1 when a batch on this table can be served by one
   scan of the packed buffer: the table is one ugpu_dfa_plan_host accepts, no
   match can contain '\n' (ugpu_tables_newline_host), and pattern_flags has no
   UGPU_PAT_EMPTY (option N's "never at the end of the input" is a per-input
   rule).  Returns what ugpu_dfa_plan_host returns. */
int ugpu_batch_plan_host(const uint32_t *opc, uint32_t nop, uint32_t pattern_flags, int *one_scan);

/* Cut a sorted device match list (as ugpu_scan_offsets writes it) at nseg + 1
   ascending device offsets d_bounds (the last <= len) into per-segment
   results; same buffer rules as ugpu_lines.  Segment s is [bounds[s],
   bounds[s+1]); empty segments, and runs of them, are allowed.  d_first[s]
   (nseg + 1 entries) = index of the first record with start >= bounds[s]:
   segment s owns the records [first[s], first[s+1]); records before bounds[0]
   or at or after bounds[nseg] belong to no segment (their rel and line are 0).
   d_cap NULL: every record has accept index cap1; d_len NULL: all lengths 0.
   Per record: d_rel = start - bounds[s], d_line = 1 + the number of '\n' in
   [bounds[s], start) (either array may be NULL).  Per segment: d_digest =
   sum(rel*31 + len) and d_dcap = sum((rel+1)*cap) mod 2^64 (ugpu_totals'
   definitions with the segment's own offsets), d_newlines = the number of '\n'
   in the segment, d_mlines = the number of distinct line values among its
   records (matching_lines of ugpu_lines over that segment alone).  Integer
   sums only: results repeat exactly from run to run.  Synchronous. */
int ugpu_split_matches(const uint8_t *dbuf, uint64_t len, const uint64_t *d_bounds, uint32_t nseg,
                       const uint64_t *d_start, const uint32_t *d_len, const uint32_t *d_cap, uint32_t cap1, uint64_t n,
                       uint64_t *d_first, uint64_t *d_digest, uint64_t *d_dcap, uint64_t *d_newlines,
                       uint64_t *d_mlines, uint64_t *d_rel, uint64_t *d_line, void *stream);

/* FIND over ninputs host buffers.  For every input i, (count, digest, dcap,
   records) equal ugpu_find_all(dfa, bufs[i], lens[i], 0, mode), and newlines,
   matching_lines and line equal ugpu_lines over that input alone (the added
   separator does not count) -- for every table ugpu_dfa_create accepts; only
   the cost differs.  The inputs are packed into pinned memory and go to the
   device in one copy per sub-batch of at most UGPU_BATCH_BYTES packed bytes
   (environment, read at each call; default 1 GiB; a sub-batch is cut only
   between inputs, a larger input is a sub-batch by itself).  A sub-batch is
   served by one scan of the packed buffer plus ugpu_split_matches when
   ugpu_batch_plan_host allows it and not both hold: the table has per-context
   accepts (ugpu_dfa_info.contexts != 1) and some input of the sub-batch ends
   in a bare '\r'.  Otherwise each input is scanned by itself over its range of
   the packed copy, and the same split lays the result out.  flags has
   UGPU_BATCH_ONE_SCAN when no sub-batch took the per-input route.  COUNT mode
   skips the record arrays (start, len, cap, line are NULL).  ninputs == 0
   gives an empty result; a NULL bufs[i] with lens[i] > 0 gives UGPU_INVAL.
   Synchronous. */
#define UGPU_BATCH_ONE_SCAN 1u
typedef struct ugpu_batch_result
{
  uint32_t ninputs, flags;
  uint64_t count;                                        /* all inputs */
  uint64_t *first;                                       /* ninputs + 1: input i's records are [first[i], first[i+1]) */
  uint64_t *digest, *dcap, *newlines, *matching_lines;   /* ninputs each */
  uint64_t *start;                                       /* count each; start is relative to its input */
  uint32_t *len, *cap;
  uint64_t *line;                                        /* 1-based line within its input */
} ugpu_batch_result;
int ugpu_find_batch(const ugpu_dfa *dfa, const uint8_t *const *bufs, const uint64_t *lens, uint32_t ninputs,
                    uint32_t mode, ugpu_batch_result **out);
int ugpu_batch_free(ugpu_batch_result *r);

/* --- binary-file detection ---
   Device buffers of any alignment (the kernel reads the enclosing 16-byte
   granules).  Synchronous. */

/* reflex::isutf8(s, s + len) (lib/simd.cpp:169-421): *first_bad = UINT64_MAX
   when the bytes are valid UTF-8 without NUL (as the reference defines it:
   surrogates and 3/4-byte overlongs pass), else the offset of the first byte
   that fails (len for a sequence cut off by the end). */
int ugpu_check_utf8(const uint8_t *dbuf, uint64_t len, uint64_t *first_bad, void *stream);

/* memchr(s, '\0', len): *pos = offset of the first NUL or UINT64_MAX. */
int ugpu_find_nul(const uint8_t *dbuf, uint64_t len, uint64_t *pos, void *stream);

/* ugrep's is_binary(s, n) (src/ugrep.cpp:699-711) and, with
   UGPU_BIN_INIT_WINDOW, GrepWorker::init_is_binary() (:3998-4015) over a
   window of len bytes (a trailing UTF-8 sequence is not judged).
   flags: UGPU_BIN_NULL_DATA = --null-data (never binary by content);
   UGPU_BIN_NUL_ONLY = -a/-U without -W (binary iff it holds a NUL);
   otherwise binary iff not isutf8. */
#define UGPU_BIN_NULL_DATA 1u
#define UGPU_BIN_NUL_ONLY 2u
#define UGPU_BIN_INIT_WINDOW 4u
int ugpu_is_binary(const uint8_t *dbuf, uint64_t len, uint32_t flags, int *binary, void *stream);

/* --- input encodings ---
   The conversion reflex::Input does in front of the matcher: UTF-16/32,
   Latin-1, the 8-bit code pages and --null-data into the UTF-8 (or swapped)
   bytes every scan and line consumer takes.  The result is, byte for byte,
   what Input::file_get (lib/input.cpp:748-1023) writes for one call with an
   unbounded n.  Its behaviour when a multi-byte sequence straddles the end of
   the caller's buffer (uidx_/ulen_, :790-797) depends on chunk sizes and has
   no counterpart.  Not reproduced either: the buffered head bytes when
   --encoding=UTF-16/32 is forced on a file without a BOM (:1307-1394), where
   the reference reads stale bytes. */
#define UGPU_ENC_PLAIN 0 /* also what ugpu_detect_bom returns for "no BOM" */
#define UGPU_ENC_UTF8 1
#define UGPU_ENC_UTF16BE 2
#define UGPU_ENC_UTF16LE 3
#define UGPU_ENC_UTF32BE 4
#define UGPU_ENC_UTF32LE 5
#define UGPU_ENC_LATIN1 6
#define UGPU_ENC_PAGE 7
#define UGPU_ENC_NULL_DATA 8

/* Input::file_init (lib/input.cpp:661-745), host only: the encoding a BOM in
   head[0, min(len, 4)) announces and the bytes to skip; len is the length of
   the whole input (head holds its first min(len, 4) bytes).
     EF BB BF                      UTF8, skip 3
     FE FF                         UTF16BE, skip 2
     FF FE 00 00                   UTF32LE, skip 4
     FF FE, len >= 4               UTF16LE, skip 2 (the reference converts the
                                   first unit inside file_init, :706-723, by
                                   the rules of the body)
     FF FE, len < 4                PLAIN, skip 0
     00 00 FE FF                   UTF32BE, skip 4
     anything else                 PLAIN, skip 0 */
int ugpu_detect_bom(const uint8_t *head, uint64_t len, uint32_t *enc, uint32_t *skip);

/* Host only: *bound = the largest output of `bytes` input bytes under enc
   (UTF-16: 5 bytes per 2; UTF-32: 5 per 4; Latin-1: 2 per 1; a code page: 3
   per 1; null data: 1 per 1).  UGPU_INVAL for PLAIN, UTF8 and unknown enc. */
int ugpu_transcode_bound(uint32_t enc, uint64_t bytes, uint64_t *bound);

/* Converts dbuf[start, len) (a device buffer, 16-byte aligned with a readable
   last granule as for ugpu_lines; start skips a BOM without breaking that
   alignment) into d_dst[0, *out_len) (device, 16-byte aligned, capacity
   bytes).  With utf8(c) = reflex::utf8(int, char*) (include/reflex/utf8.h:
   76-135: 1-4 bytes by the usual ranges, D800..DFFF not rejected (3 bytes),
   c > 0x10FFFF the five bytes F8 88 80 80 80 of REFLEX_NONCHAR):
     UTF16BE/LE (:770-847)  units u[0, floor(n / 2)), a trailing odd byte is
        dropped.  A unit in D800..DBFF (H) always consumes the unit behind it:
        it emits utf8(0x10000 + ((u[i] - 0xD800) << 10) + (u[i+1] - 0xDC00))
        when that unit exists and lies in DC00..DFFF, NONCHAR otherwise, and
        the consumed unit emits nothing whatever it is.  A unit in DC00..DFFF
        that is not consumed emits NONCHAR; any other unit emits utf8(u[i]).
     UTF32BE/LE (:848-909)  per 4 bytes, c a signed 32-bit int: c < 0x80
        (negative values included) emits the byte c & 0xFF, otherwise utf8(c);
        a trailing 1-3 bytes are dropped.
     LATIN1 (:910-938)      a byte < 0x80 unchanged, otherwise utf8(byte).
     PAGE (:939-1000)       c = page[byte], the 256-entry table
        Input::file_encoding(enc, page) receives (host memory): c < 0x80 one
        byte, otherwise utf8(c).
     NULL_DATA (:1001-1016) '\0' and '\n' swapped.
   d_dst NULL is a size query: the summary pass only, *out_len valid.  When
   *out_len > capacity the call returns UGPU_CAPACITY with *out_len valid and
   nothing written; otherwise only d_dst[0, *out_len) is written.  UGPU_INVAL,
   decided before the device is touched: an unknown enc, PLAIN or UTF8 (nothing
   to convert), PAGE without a page or a page with another enc, start > len.
   len == start is valid and gives 0.  Offsets are 64-bit throughout (a 2.2 GiB
   Latin-1 input gives more than 4 GiB).  Synchronous. */
int ugpu_transcode(const uint8_t *dbuf, uint64_t len, uint64_t start, uint32_t enc, const uint16_t *page,
                   uint8_t *d_dst, uint64_t capacity, uint64_t *out_len, void *stream);

/* --- file indexes ---
   The pass ugrep-indexer makes over every file (src/ugrep-indexer.cpp:
   805-1030) so that ugrep --index can skip files that cannot match.  Per input:
     table   65536 bytes of 0xff; for every position i and k in 0..7 with
             i + k < n, bit k of table[h(i, k)] is cleared, h(i, 0) = byte[i],
             h(i, k) = (61 h(i, k-1) + byte[i+k]) mod 2^16 (indexhash, :806-809;
             the 64 KiB reads, the 8-byte window and the tail loop of :928-977
             come to this set of (i, k))
     fold    size = 65536; while size > 128: z = the zero bits of the AND of
             the two halves; stop when 100 z >= max_noise * 8 * (size / 2),
             otherwise that AND is the table and size halves (:997-1027, in
             float there; z < 2^24 and the divisors are powers of two, so the
             integer comparison decides the same).  max_noise by accuracy
             0..9: 80 73 65 57 49 42 34 26 18 10 (noise_percentage, :266-270)
     binary  over the first min(n, 65536) bytes, the window's last UTF-8
             sequence cut off first (:892-901), then is_binary (:782-803): a
             NUL, a lead outside C2..F4 or a lead without its continuation
             bytes.  This is not reflex::isutf8: surrogates and 3/4-byte
             overlongs pass.
   The header byte of an input's record (:1725-1731) is log2(size) | binary << 7;
   an empty input, and a binary one under UGPU_INDEX_IGNORE_BINARY (-I), has
   log2 0 and no table.  The bytes to pass are those reflex::Input delivers
   (ugpu_detect_bom / ugpu_transcode for a file with a BOM).  Archives,
   decompression, --check, --delete and incremental updates are not here.  The
   query over these tables (Pattern::match_hfa) is ugpu_index_query below. */
#define UGPU_INDEX_IGNORE_BINARY 1u

/* The bytes of an input one workgroup hashes: an input of up to this many
   bytes is hashed, folded and counted in one workgroup, a longer one is cut
   into chunks of this size whose tables meet in global memory. */
uint64_t ugpu_index_chunk(void);

/* Indexes the nseg segments [bounds[s], bounds[s+1]) of dbuf[0, len) (a device
   buffer, 16-byte aligned with a readable last granule as for ugpu_lines;
   bounds: nseg + 1 ascending host values, bounds[nseg] <= len; segments lie
   back to back or apart, and no window reads past its segment's end).  Host
   outputs: header[s] as above, zero_bits[s] the zero bits of the final table
   (ugrep-indexer -v prints 100 zero_bits / (8 size), rounded), offset[s] the
   place of its 1 << (header[s] & 31) table bytes (none when that log2 is 0) in
   d_tables, offset[nseg] = *tables_len.  The tables lie compactly in segment
   order in d_tables (device, 16-byte aligned, capacity bytes).  d_tables NULL
   is a size query.  When *tables_len > capacity the call returns
   UGPU_CAPACITY with every host output valid; d_tables then holds the tables
   of some leading segments.  A final table has at most max(128, the smallest
   power of two above 100 n / max_noise) bytes, which bounds a capacity without
   a query.  UGPU_INVAL, decided before the device is touched: accuracy > 9, an
   unknown flag, bounds that descend or pass len.  nseg == 0 gives
   *tables_len = 0.  The device workspace for tables is bounded (256 MiB;
   segments go in groups).  Synchronous. */
int ugpu_index_tables(const uint8_t *dbuf, uint64_t len, const uint64_t *bounds, uint32_t nseg, uint32_t accuracy,
                      uint32_t flags, uint8_t *header, uint32_t *zero_bits, uint64_t *offset, uint8_t *d_tables,
                      uint64_t capacity, uint64_t *tables_len, void *stream);

/* ugpu_index_tables over host inputs: packed back to back, with no separator
   bytes, through pinned memory, in sub-batches cut between inputs as for
   ugpu_find_batch.  Zero-length inputs are legal anywhere; ninputs == 0 gives
   an empty result; accuracy > 9 and a NULL bufs[i] with lens[i] > 0 give
   UGPU_INVAL.  The arrays of the result are malloc'd and freed by
   ugpu_index_free: header and zero_bits per input, offset[ninputs + 1] into
   tables. */
typedef struct ugpu_index_result
{
  uint32_t ninputs;
  uint32_t accuracy;
  uint8_t *header;
  uint32_t *zero_bits;
  uint64_t *offset;
  uint8_t *tables;
} ugpu_index_result;
int ugpu_index_batch(const uint8_t *const *bufs, const uint64_t *lens, uint32_t ninputs, uint32_t accuracy,
                     uint32_t flags, ugpu_index_result **out);
int ugpu_index_free(ugpu_index_result *r);

/* --- the index query: which records may match ---
   ugrep --index compiles its pattern with option h (src/ugrep.cpp:8849) into a
   "hash finite automaton" and asks it, per record of a ._UG#_Store, whether
   the file can match; a file that cannot is not opened.

   ugpu_hfa_create replaces Pattern::gen_match_hfa, gen_match_hfa_start and
   gen_match_hfa_transitions (lib/pattern.cpp:4641-4755).  For every DFA state
   reachable in level + 1 bytes from the start, level 0..15, and every offset
   in max(0, level - 7)..level, it keeps the set of hashes (indexhash,
   include/reflex/pattern.h:1284: h' = (61 h + b) mod 2^16, the indexer's) of
   the byte chains that begin at depth `offset` and end with the state's
   incoming byte, and the state's successors.  A state without successors is
   "dead", which means accept: one that accepts, has no edges, or whose lowest
   edge leads to such a state (:4687 with next_accepting, pattern.h:740-745,
   looks at that edge alone).  It is built from the native compiler's subset
   DFA before minimisation (the reference's DFA is not minimised either), with
   `flags` the UGPU_RX_* of ugpu_compile.  Assertions at a pattern's ends (the
   reference's meta edges, which its closure skips) are dropped: a superset
   language.  A construct the native compiler refuses gives UGPU_UNSUPPORTED
   (message in ugpu_last_error); the caller then keeps every file.  A pattern
   whose start state accepts or has no edges (a*) has no automaton
   (Pattern::has_hfa false, src/ugrep.cpp:8931): every file is kept.
   The reference truncates an automaton of more than 1024 states or 262144
   ranges per state in the order of its states' addresses (:4695, :4748); here
   generation stops when the 1024 state ids or 4 Mi ranges run out and every
   entry of the last level is dead, which keeps more files and never fewer, and
   parity is not claimed (info.truncated). */
typedef struct ugpu_hfa ugpu_hfa;
typedef struct ugpu_hfa_info_t
{
  uint32_t has_hfa;   /* 0: no automaton, every file is kept */
  uint32_t levels;    /* levels with entries, up to 16 */
  uint32_t states;    /* distinct states among the entries */
  uint32_t entries;   /* (state, level) pairs */
  uint32_t ranges;    /* hash ranges over all entries and offsets */
  uint32_t truncated; /* cut short: looser than the reference may be */
  uint64_t hashes;    /* hashes in those ranges */
} ugpu_hfa_info_t;
int ugpu_hfa_create(const char *regex, size_t len, uint32_t flags, ugpu_hfa **hfa);
int ugpu_hfa_destroy(ugpu_hfa *hfa);
int ugpu_hfa_info(const ugpu_hfa *hfa, ugpu_hfa_info_t *info);
/* The flattened automaton as 32-bit words (layout: ugrep_amd/csrc/hfa.hpp):
   export with words NULL is a size query (0 words: no automaton); import
   checks every index and returns UGPU_INVAL for words it cannot follow. */
int ugpu_hfa_export(const ugpu_hfa *hfa, uint32_t *words, uint64_t capacity, uint64_t *nwords);
int ugpu_hfa_import(const uint32_t *words, uint64_t nwords, ugpu_hfa **hfa);

/* Pattern::match_hfa and match_hfa_transitions (lib/pattern.cpp:4757-4815)
   over one table of `size` bytes (a power of two up to 65536), host only:
   *keep = 1 when the file may match.  Levels run in order with two visit sets
   that alternate by level & 1 and are never cleared (a state seen at an
   earlier depth of the same parity stays visited); level 0 tests every entry.
   A visited entry passes an offset when some hash h of that set has bit
   level - offset clear in table[h & (size - 1)].  Offsets are tried in
   ascending order up to the first that fails; each one that passes marks the
   entry's successors for the next level, so an entry propagates iff its first
   offset passes, and a dead entry whose first offset passes ends the query
   with keep.  A level on which no entry passes all its offsets ends it with
   skip.  Without an automaton *keep = 1. */
int ugpu_hfa_match_host(const ugpu_hfa *hfa, const uint8_t *table, uint64_t size, int *keep);
/* The decision per record (see ugpu_index_query) on the host, tables in host
   memory: the fallback without a device.  Without an automaton every byte of
   keep is 1, whatever the headers say. */
int ugpu_hfa_query_host(const ugpu_hfa *hfa, const uint8_t *tables, const uint8_t *header, const uint64_t *offset,
                        uint32_t nrec, uint32_t flags, uint8_t *keep);

/* The decision per record (src/ugrep.cpp:10060-10099), on the device.  header,
   offset (nrec + 1 values) and d_tables lie as ugpu_index_tables leaves them
   (header and offset in host memory, d_tables a device buffer).  With
   b = header[s]: b & 0x80 under UGPU_QUERY_IGNORE_BINARY (-I) skips; b & 0x60
   (an archive or a compressed file) without UGPU_QUERY_DECOMPRESS (-z) skips;
   a table (b & 0x1F != 0) keeps iff the automaton does; no table keeps iff
   b & 0x80.  keep (host, nrec bytes) gets 0 = skip, 1 = keep.  Without an
   automaton every byte is 1 and nothing is launched.  A table must lie inside
   [0, offset[nrec]) at its offset, else UGPU_INVAL before the device is touched.
   One wave walks one record; a table of up to ugpu_index_query_lds() bytes is
   staged in LDS first, a larger one is probed in global memory (the
   UGPU_QUERY_FORCE_* flags pin either way, for tests and measurements).
   The automaton's words are uploaded when the pooled workspace that serves the
   call last served another ugpu_hfa (a copy per workspace, not per ugpu_hfa).
   Synchronous. */
#define UGPU_QUERY_IGNORE_BINARY 1u
#define UGPU_QUERY_DECOMPRESS 2u
#define UGPU_QUERY_FORCE_LDS 0x100u    /* stage every table (up to 65536 bytes) */
#define UGPU_QUERY_FORCE_GLOBAL 0x200u /* stage none */
int ugpu_index_query(const ugpu_hfa *hfa, const uint8_t *d_tables, const uint8_t *header,
                     const uint64_t *offset, uint32_t nrec, uint32_t flags, uint8_t *keep, void *stream);
uint32_t ugpu_index_query_lds(void);
/* ugpu_index_query over tables in host memory, compact as ugpu_index_batch
   returns them (offsets ascending): they go through pinned memory in
   sub-batches cut between records. */
int ugpu_index_query_records(const ugpu_hfa *hfa, const uint8_t *tables, const uint8_t *header, const uint64_t *offset,
                             uint32_t nrec, uint32_t flags, uint8_t *keep);
/* The device time (hipEvents around the kernels, ms) of this thread's last
   ugpu_index_query, ugpu_index_query_records or ugpu_index_query_store. */
int ugpu_index_query_kernel_ms(float *ms);

/* ugpu_index_query over nblobs index stores as read from disk (host memory):
   the records are parsed on the host (the magic, then per record the accuracy
   digit, the header byte, the name's length in 16 bits, the name, the table),
   the tables go through pinned memory in sub-batches and the result holds one
   keep byte per record with its name's place: name_blob[i], name_off[i],
   name_len[i].  UGPU_INVAL for a blob without the magic or with a cut record.
   Freed by ugpu_query_free. */
typedef struct ugpu_query_result
{
  uint32_t nrec;
  uint8_t *keep;
  uint8_t *header;
  uint32_t *name_blob;
  uint64_t *name_off;
  uint32_t *name_len;
} ugpu_query_result;
int ugpu_index_query_store(const ugpu_hfa *hfa, const uint8_t *const *blobs, const uint64_t *lens, uint32_t nblobs,
                           uint32_t flags, ugpu_query_result **out);
int ugpu_query_free(ugpu_query_result *r);

/* --- synthetic corpora, generated on device --- */
#define UGPU_GEN_WORDS 1
#define UGPU_GEN_PLANTED 2
#define UGPU_GEN_CODE 3
#define UGPU_GEN_UTF8 4
/* Write bytes [off, off+len) of corpus `kind` with `seed` into dbuf. */
int ugpu_gen(int kind, uint64_t seed, uint64_t off, uint8_t *dbuf, uint64_t len, void *stream);

/* --- regex -> opcode words (replaces Matcher::convert + Pattern(conv, "r"),
   lib/convert.cpp and lib/pattern.cpp:171-3063, for FIND tables) ---

   Compiles `regex` (len bytes, ugrep's default ERE syntax in Unicode mode with
   notnewline, src/ugrep.cpp:8574-8578) into opcode words in the reference's
   format (include/reflex/pattern.h:1155-1247), language-equivalent per accept
   index to the reference's Pattern; feed them to ugpu_dfa_create().  *opc is
   malloc'd, free it with ugpu_opc_free().  Returns UGPU_INVAL on a syntax error
   (the reference throws regex_error, lib/pattern.cpp:162-169) and
   UGPU_UNSUPPORTED for constructs the GPU tables do not cover (anchors, word
   boundaries, lazy quantifiers, lookaround, rare \p{..} scripts, \p{Lu} under -i); the
   message is in ugpu_compile_error(). */
#define UGPU_RX_FIXED 1u /* -F: the pattern is a literal string (src/cnf.hpp:147-165) */
#define UGPU_RX_ICASE 2u /* -i: ASCII letters and the reference's Unicode case pairs */
/* The regex a reflex::Pattern holds (its public Pattern::operator[](0),
   include/reflex/pattern.h:302): RE/flex syntax over bytes as produced by
   Matcher::convert (lib/convert.cpp) -- Unicode classes, '.' and -i over
   non-ASCII letters already expanded into byte sequences; inline (?i) (?s) (?m)
   modifiers and (?i:...) scopes; \Q...\E.  The drop-in adapter builds its tables
   from this, so it needs no access to Pattern's private opcode words. */
#define UGPU_RX_REFLEX 4u
int ugpu_compile(const char *regex, size_t len, uint32_t flags, uint32_t **opc, uint32_t *nop);
void ugpu_opc_free(uint32_t *opc);
const char *ugpu_compile_error(void);

const char *ugpu_last_error(void);
const char *ugpu_version(void);
/* Provenance of the device library: "src:<hash of ugrep_amd/csrc and this
   header (tools/srchash.py)> git:<commit it was built at>".  The Python
   binding warns when the hash differs from the sources beside the library. */
const char *ugpu_build_id(void);
/* UGPU_ABI_VERSION of the header the library was built with */
int ugpu_abi_version(void);

/* Devices (no reference counterpart: its matchers are CPU threads).
   ugpu_select_device makes `dev` the calling thread's device (hipSetDevice):
   ugpu_find_all, ugpu_stream_create and scanners created afterwards on this
   thread run there, with the table copy a ugpu_dfa keeps per device (uploaded
   at the first use).  The drop-in adapter spreads ugrep's worker matchers over
   the devices this way. */
int ugpu_device_count(int *n);
int ugpu_select_device(int dev);
/* Initialise device dev for this process ahead of its first scan: the HIP
   context, a scan and a records workspace (streams), a pinned block, the
   kernels' code object -- the ~0.2-0.4 s a fresh process pays at its first
   GPU call (tools/probe/startup_probe.cpp).  The drop-in matcher runs it on a
   thread of its own while the CPU matcher serves the first inputs. */
int ugpu_warmup(int dev);

#ifdef __cplusplus
}
#endif

#endif /* UGPU_H */
