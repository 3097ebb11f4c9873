// linebool.hip -- Boolean line queries on the device: which lines satisfy a
// CNF over several match lists (ugrep --bool, -e A --and B --andnot C, --not,
// --files).
//
// Replaces, for a fully buffered input, ugrep's per-line CNF check
// (cnf_matching, src/ugrep.cpp:3277-3376: one sub-matcher find() per literal
// over each candidate line; cnf_satisfied, :3379-3427, for --files).  Here
// every sub-pattern has scanned the whole buffer once and left a sorted match
// list; one line pass turns the K lists into per-line literal bits and
// evaluates the formula for 32 lines per integer operation.
//
// The passes, wave ranges, tiles and host stitching are those of linesel.hip
// (the steps of the walk are shared through line_select.hpp, the host driver
// through line_host.hpp), with K lists in place of one:
//
//   bool_summary_kernel  per wave: 1 + position of the last '\n' of its range
//                        and, per list, the largest exclusive end of the
//                        matches starting in the range;
//   (host)               prefix sum of the newline counts, prefix max of the
//                        others: line number, line begin and K covers at every
//                        range start; with UGPU_BOOL_FILES the final covers are
//                        the whole-input literals and the formula is decided
//                        here, leaving "the lines any list touches" or nothing
//                        for the line passes;
//   bool_kernel<false>   per wave: number of selected lines it owns;
//   (host)               exclusive prefix of those counts;
//   bool_kernel<true>    the same walk, writing (begin, end, lineno).
//
// bool_kernel keeps one line bitmap per list in LDS (kTbWords words each, all
// K at once: the formula is then read clause by clause without a second walk
// of the lists).  Per tile every list marks the lines its matches touch, its
// carried cover included; then each lane takes words of the bitmaps, computes
//   acc = ~0; for each clause: acc &= OR_{t in pos} tb[t][w] | OR_{t in neg} ~tb[t][w]
// and stores the word, xored for UGPU_SEL_INVERT, over bitmap 0, from which
// the per-granule fields, scans and record writes go on as in sel_kernel.
// The kernel is built for 4 and for 16 bitmaps (12.6 and 38.5 KiB of LDS per
// block), chosen by the number of lists the formula uses.
#include "device_common.hpp"
#include "line_host.hpp"
#include "line_select.hpp"

namespace ugpu {

namespace {

__device__ __forceinline__ uint64_t uni64(uint64_t v)
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

// the formula over one line's (or, on the host, the whole input's) literal bits
__host__ __device__ __forceinline__ bool formula(const BoolParams& S, uint32_t bits)
{
  if (!S.all) return false;
  for (uint32_t c = 0; c < S.ncl; ++c)
    if (!((bits & S.pos[c]) | (~bits & S.neg[c]))) return false;
  return true;
}

// the formula over word w of the wave's bitmaps: 32 lines at once
template <int KMAX>
__device__ __forceinline__ uint32_t eval_word(const BoolParams& S, const uint32_t* tb, uint32_t w)
{
  uint32_t v[KMAX];
#pragma unroll
  for (int t = 0; t < KMAX; ++t) v[t] = (uint32_t)t < S.nl ? tb[t * kTbWords + w] : 0u;
  uint32_t acc = S.all;
  for (uint32_t c = 0; c < S.ncl; ++c) {
    const uint32_t p = S.pos[c], q = S.neg[c];
    uint32_t o = 0;
#pragma unroll
    for (int t = 0; t < KMAX; ++t) o |= (v[t] & (0u - ((p >> t) & 1u))) | (~v[t] & (0u - ((q >> t) & 1u)));
    acc &= o;
  }
  return S.invert ? ~acc : acc;
}

}  // namespace

__global__ __launch_bounds__(kSWaves * 64) void bool_summary_kernel(BoolParams S)
{
  const int lane = threadIdx.x & 63;
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (gw >= S.nwaves) return;
  const SRange r = srange(S.len, S.per, gw);
  const uint64_t last = last_newline(S.g, r, lane);
  if (lane == 0) S.lastnl[gw] = last;
  for (uint32_t t = 0; t < S.nl; ++t) {
    const uint64_t cv = range_cover(S.starts[t], S.lens[t], S.nmatch[t], S.len, r, lane);
    if (lane == 0) S.mcover[(uint64_t)t * S.nwaves + gw] = cv;
  }
}

template <bool WRITE, int KMAX>
__global__ __launch_bounds__(kSWaves * 64) void bool_kernel(BoolParams S)
{
  __shared__ uint16_t gmask[kSWaves][256], gpre[kSWaves][256];
  __shared__ uint32_t tbits[kSWaves][KMAX * kTbWords];
  // per list: index of the next match to place, its start (~0: none left) and
  // the exclusive end of the bytes touched by the matches before it
  __shared__ uint64_t lnext[kSWaves][KMAX], lstart[kSWaves][KMAX], lcover[kSWaves][KMAX];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + wid;
  if (gw >= S.nwaves) return;
  const SRange r = srange(S.len, S.per, gw);
  uint16_t* gm = gmask[wid];
  uint16_t* gp = gpre[wid];
  uint32_t* tb = tbits[wid];
  uint64_t* nx = lnext[wid];
  uint64_t* ns = lstart[wid];
  uint64_t* cv = lcover[wid];
  const uint32_t nl = S.nl < (uint32_t)KMAX ? S.nl : (uint32_t)KMAX;
  for (uint32_t t = 0; t < nl; ++t) {
    const uint64_t n = S.nmatch[t];
    const uint64_t j = lower64(S.starts[t], n, r.lo, lane);
    if (lane == 0) {
      nx[t] = j;
      ns[t] = j < n ? S.starts[t][j] : ~0ull;
      cv[t] = S.cover[(uint64_t)t * S.nwaves + gw];
    }
  }
  uint64_t line = 1 + S.prefix[gw];  // line of byte r.lo
  uint64_t bol = S.bol[gw];          // begin of that line
  uint64_t out = WRITE ? S.obase[gw] : 0;
  uint32_t nsel = 0;                 // (count pass) selected lines, per lane
  const uint32_t nzero = (nl ? nl : 1u) * (uint32_t)kTbWords;
  for (uint32_t i = 0; i < r.n; ++i) {
    wave_sync();  // the previous tile's LDS reads precede these writes
    const uint64_t ts = r.lo + (uint64_t)i * kSTile;
    const uint64_t tend = ts + kSTile < r.hi ? ts + kSTile : r.hi;
    uint32_t c[4];
    for (uint32_t w = lane; w < nzero; w += 64) tb[w] = 0;
    const uint32_t base = tile_masks(S.g, r, i, lane, gm, gp, c);
    wave_sync();
    for (uint32_t t = 0; t < nl; ++t) {
      uint32_t* tbt = tb + t * (uint32_t)kTbWords;
      uint64_t cover = uni64(cv[t]);
      mark_cover(tbt, gm, gp, cover, bol, ts, tend, lane);
      if (uni64(ns[t]) >= tend) continue;  // no match of this list starts in the tile
      const uint64_t* starts = S.starts[t];
      const uint32_t* lens = S.lens[t];
      const uint64_t n = S.nmatch[t];
      uint64_t cl;
      const uint64_t j = place_matches(tbt, gm, gp, starts, lens, n, S.len, uni64(nx[t]), ts, tend, lane, cl);
      cl = wave_max(cl);
      cover = cl > cover ? cl : cover;
      if (lane == 0) {
        nx[t] = j;
        ns[t] = j < n ? starts[j] : ~0ull;
        cv[t] = cover;
      }
    }
    wave_sync();
    // the formula, 32 lines per word, over bitmap 0 (a lane reads its word of every list first)
    for (uint32_t w = lane; w < (uint32_t)kTbWords; w += 64) tb[w] = eval_word<KMAX>(S, tb, w);
    wave_sync();
    // the lines ending in this tile, per granule: their bits and 1 + tile offset of its last newline
    uint32_t field[4], lp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t g = 64u * k + lane;
      field[k] = granule_field(tb, gp[g], c[k], 0u);
      lp[k] = last_in_granule(gm, g);
    }
    if (WRITE) {
      uint32_t selbase = 0, lastp = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t g = 64u * k + lane;
        const uint32_t sc = __popc(field[k]);
        const uint32_t incl = lscan_add(sc);
        const uint32_t inclp = lscan_max(lp[k]);
        const uint32_t up = (uint32_t)__shfl_up((int)inclp, 1, 64);
        const uint32_t prevp = umax(lane ? up : 0u, lastp);  // 1 + tile offset of the last newline before g
        uint64_t b = prevp ? ts + prevp : bol;
        uint64_t slot = out + selbase + incl - sc;
        uint64_t ln = line + gp[g];
        uint32_t mm = gm[g], f = field[k];
        while (mm) {
          const uint64_t p = ts + 16u * g + (uint32_t)__builtin_ctz(mm);
          if (f & 1u) {
            S.begin[slot] = b;
            S.end[slot] = p;
            S.lineno[slot] = ln;
            ++slot;
          }
          b = p + 1;
          ++ln;
          f >>= 1;
          mm &= mm - 1u;
        }
        selbase += (uint32_t)__builtin_amdgcn_readlane(incl, 63);
        lastp = umax(lastp, (uint32_t)__builtin_amdgcn_readlane(inclp, 63));
      }
      out += selbase;
    } else {
      nsel += __popc(field[0]) + __popc(field[1]) + __popc(field[2]) + __popc(field[3]);
    }
    if (base) {  // the line open after this tile begins behind its last newline
#pragma unroll
      for (int k = 3; k >= 0; --k) {
        const uint64_t bm = __ballot(c[k] != 0);
        if (bm) {
          bol = ts + (uint32_t)__shfl((int)lp[k], 63 - __builtin_clzll(bm), 64);
          break;
        }
      }
      line += base;
    }
  }
  uint64_t total = WRITE ? 0 : wave_sum((uint64_t)nsel);
  if (gw == S.nwaves - 1 && bol < S.len) {  // the unterminated last line
    wave_sync();
    uint32_t bits = 0;
    for (uint32_t t = 0; t < nl; ++t)
      if (uni64(cv[t]) > bol) bits |= 1u << t;
    if (formula(S, bits) != (S.invert != 0))
      tail_line<WRITE>(bol, S.len, line, out, lane, S.begin, S.end, S.lineno, total);
  }
  if (!WRITE && lane == 0) S.selcnt[gw] = total;
}

hipError_t launch_bool_summary(const BoolParams& S, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((S.nwaves + kSWaves - 1) / kSWaves);
  hipLaunchKernelGGL(bool_summary_kernel, dim3(grid), dim3(kSWaves * 64), 0, stream, S);
  return hipGetLastError();
}

hipError_t launch_bool(const BoolParams& S, bool write, hipStream_t stream)
{
  const dim3 grid((uint32_t)((S.nwaves + kSWaves - 1) / kSWaves)), block(kSWaves * 64);
  if (S.nl <= 4) {
    if (write)
      hipLaunchKernelGGL((bool_kernel<true, 4>), grid, block, 0, stream, S);
    else
      hipLaunchKernelGGL((bool_kernel<false, 4>), grid, block, 0, stream, S);
  } else {
    if (write)
      hipLaunchKernelGGL((bool_kernel<true, (int)kBoolLists>), grid, block, 0, stream, S);
    else
      hipLaunchKernelGGL((bool_kernel<false, (int)kBoolLists>), grid, block, 0, stream, S);
  }
  return hipGetLastError();
}

}  // namespace ugpu

// ---------------------------------------------------------------- C ABI
using namespace ugpu;

static_assert(UGPU_BOOL_MAX_LISTS == kBoolLists && UGPU_BOOL_MAX_CLAUSES == kBoolClauses, "ugpu.h limits");

int ugpu_select_lines_bool(const uint8_t* dbuf, uint64_t len, const uint64_t* const* d_starts,
                           const uint32_t* const* d_lens, const uint64_t* n, uint32_t nlists,
                           const ugpu_bool_clause* clauses, uint32_t nclauses, uint32_t flags, uint64_t* d_begin,
                           uint64_t* d_end, uint64_t* d_lineno, uint64_t capacity, uint64_t* selected, uint64_t* lines,
                           int* whole, void* stream)
{
  if (!dbuf || (nlists && !(d_starts && n)) || (nclauses && !clauses)) return fail(UGPU_INVAL, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dbuf) & 15u) return fail(UGPU_INVAL, "buffer must be 16-byte aligned");
  if (flags & ~(UGPU_SEL_INVERT | UGPU_BOOL_FILES)) return fail(UGPU_INVAL, "unknown flags");
  if (nlists > UGPU_BOOL_MAX_LISTS) return fail(UGPU_INVAL, "more than UGPU_BOOL_MAX_LISTS match lists");
  if (nclauses > UGPU_BOOL_MAX_CLAUSES) return fail(UGPU_INVAL, "more than UGPU_BOOL_MAX_CLAUSES clauses");
  const uint32_t listmask = (1u << nlists) - 1u;
  uint32_t used = 0;
  for (uint32_t c = 0; c < nclauses; ++c) {
    if ((clauses[c].pos | clauses[c].neg) & ~listmask) return fail(UGPU_INVAL, "clause names a list >= nlists");
    if (!(clauses[c].pos | clauses[c].neg)) return fail(UGPU_INVAL, "empty clause");
    used |= clauses[c].pos | clauses[c].neg;
  }
  for (uint32_t t = 0; t < nlists; ++t)
    if (n[t] && !d_starts[t]) return fail(UGPU_INVAL, "NULL match list");
  const bool files = (flags & UGPU_BOOL_FILES) != 0;
  if (files) used = listmask;  // every list: the whole-input literals and the lines any list touches
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // the lists the formula uses, renumbered from 0, and the clauses over them
  BoolParams S{};
  uint32_t slot[UGPU_BOOL_MAX_LISTS] = {};
  for (uint32_t t = 0; t < nlists; ++t)
    if (used >> t & 1u) {
      slot[t] = S.nl;
      S.starts[S.nl] = d_starts[t];
      S.lens[S.nl] = d_lens ? d_lens[t] : nullptr;
      S.nmatch[S.nl] = n[t];
      ++S.nl;
    }
  for (uint32_t c = 0; c < nclauses; ++c)
    for (uint32_t t = 0; t < nlists; ++t) {
      if (clauses[c].pos >> t & 1u) S.pos[c] |= 1u << slot[t];
      if (clauses[c].neg >> t & 1u) S.neg[c] |= 1u << slot[t];
    }
  S.ncl = nclauses;
  S.all = ~0u;
  S.invert = flags & UGPU_SEL_INVERT;
  S.g = dbuf;
  S.len = len;
  S.begin = d_begin;
  S.end = d_end;
  S.lineno = d_lineno;
  const uint32_t ncover = S.nl;
  // with UGPU_BOOL_FILES: a list with a match starting below len touches a
  // line, so the final covers are the whole-input literals
  auto decide = [&](const uint64_t* cover) {
    if (!files) return -1;
    uint32_t bits = 0;
    for (uint32_t t = 0; t < ncover; ++t)
      if (cover[t]) bits |= 1u << t;
    const int truth = formula(S, bits) ? 1 : 0;
    S.ncl = 0;
    if (truth && S.nl) {  // the lines any list touches
      S.ncl = 1;
      S.pos[0] = listmask;
      S.neg[0] = 0;
    } else {  // nothing
      S.all = 0;
      S.nl = 0;
    }
    return truth;
  };
  return select_lines_driver(
      S, ncover, capacity, selected, lines, whole, st, [&] { return launch_bool_summary(S, st); }, decide,
      [&](bool write) { return launch_bool(S, write, st); });
}
