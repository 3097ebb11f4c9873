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
// (helpers shared through line_tiles.hpp), with K lists in place of one:
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
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/ugpu.h"
#include "device_common.hpp"
#include "line_tiles.hpp"
#include "plan.hpp"

namespace ugpu {

namespace {

__device__ __forceinline__ uint64_t uni64(uint64_t v)
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

// Exclusive end of the bytes a match (start s < len, length lens[idx]) touches:
// a zero-length match touches byte s.
__device__ __forceinline__ uint64_t bmatch_end(const uint32_t* lens, uint64_t len, uint64_t idx, uint64_t s)
{
  const uint64_t l = lens ? (uint64_t)lens[idx] : 0ull;
  const uint64_t e = l ? s + l : s + 1;
  return e < len ? e : len;
}

// the formula over one line's literal bits
__device__ __forceinline__ bool formula(const BoolParams& S, uint32_t bits)
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
  uint64_t last = 0;  // 1 + position of the range's last newline
  for (uint32_t i = r.n; i-- > 0;) {
    const __amdgpu_buffer_rsrc_t rs = ltile(S.g + r.lo, i, r.rel16);
    uint32_t best = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t o = 16u * lane + 1024u * k;
      const uint32_t m = nl16(sload16(rs, o)) & granule_valid(r.rel, i * (uint32_t)kSTile + o);
      if (m) best = umax(best, o + 32u - (uint32_t)__builtin_clz(m));
    }
    best = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max(best));
    if (best) {
      last = r.lo + (uint64_t)i * kSTile + best;
      break;
    }
  }
  if (lane == 0) S.lastnl[gw] = last;
  for (uint32_t t = 0; t < S.nl; ++t) {
    const uint64_t* starts = S.starts[t];
    const uint32_t* lens = S.lens[t];
    const uint64_t n = S.nmatch[t];
    const uint64_t j0 = lower64(starts, n, r.lo, lane), j1 = lower64(starts, n, r.hi, lane);
    uint64_t cv = 0;
    for (uint64_t idx = j0 + (uint64_t)lane; idx < j1; idx += 64) {
      const uint64_t e = bmatch_end(lens, S.len, idx, starts[idx]);
      cv = e > cv ? e : cv;
    }
    cv = wave_max(cv);
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
      // the open line and the lines after it that earlier matches of this list reach
      if (cover > bol && lane == 0) {
        uint32_t hr = 0;
        if (cover > ts) hr = rank_of(gm, gp, (uint32_t)((cover < tend ? cover : tend) - 1 - ts));
        mark(tbt, 0, hr);
      }
      if (uni64(ns[t]) >= tend) continue;  // no match of this list starts in the tile
      const uint64_t* starts = S.starts[t];
      const uint32_t* lens = S.lens[t];
      const uint64_t n = S.nmatch[t];
      uint64_t j = uni64(nx[t]);
      uint64_t cl = 0;  // this lane's share of the tile's cover
      for (;;) {        // matches starting in this tile, 64 at a time
        const uint64_t idx = j + (uint64_t)lane;
        const uint64_t s = idx < n ? starts[idx] : ~0ull;
        const bool in = s < tend;
        const uint64_t mb = __ballot(in);
        if (!mb) break;
        uint32_t r0 = 0, r1 = 0;
        if (in) {
          const uint64_t e = bmatch_end(lens, S.len, idx, s);
          cl = e > cl ? e : cl;
          r0 = rank_of(gm, gp, (uint32_t)(s - ts));
          r1 = rank_of(gm, gp, (uint32_t)((e < tend ? e : tend) - 1 - ts));
        }
        // (matches crowd on a line: one whose only line the lane below has just reached leaves the bit to it)
        const uint32_t pr1 = (uint32_t)__shfl_up((int)r1, 1, 64);
        if (in && !(lane && r0 == r1 && pr1 == r0)) mark(tbt, r0, r1);
        const uint32_t k = (uint32_t)__popcll(mb);
        j += k;
        if (k < 64) break;
      }
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
    // the lines ending in this tile: granule g's are ranks gp[g] .. gp[g] + c - 1
    uint32_t field[4], lp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t g = 64u * k + lane, r0 = gp[g], m = gm[g];
      const uint64_t two = (uint64_t)tb[r0 >> 5] | ((uint64_t)tb[(r0 >> 5) + 1] << 32);
      field[k] = (uint32_t)(two >> (r0 & 31u)) & ((1u << c[k]) - 1u);
      lp[k] = m ? 16u * g + 32u - (uint32_t)__builtin_clz(m) : 0u;  // 1 + tile offset of its last newline
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
    const bool sel = formula(S, bits) != (S.invert != 0);
    if (sel) {
      if (WRITE) {
        if (lane == 0) {
          S.begin[out] = bol;
          S.end[out] = S.len;
          S.lineno[out] = line;
        }
      } else {
        ++total;
      }
    }
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

namespace {

int fail(int code, const std::string& msg) { return ugpu::host_fail(code, msg); }

int hip_fail(hipError_t e, const char* what)
{
  return ugpu::host_fail(UGPU_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// Per-call scratch, pooled per device as linesel.hip's SelWs: per wave, the
// (3 + K) arrays the kernels write (newline counts, last newline, K match
// covers, selected counts), the (3 + K) the host stitches for them (newline
// prefix, line begin, K covers, output offset), sized for K = 16, and pinned
// host copies of both.
constexpr uint64_t kSlots = 3 + kBoolLists;
constexpr uint64_t kSlotLast = 2 + kBoolLists;  // selected counts / output offsets

struct BoolWs {
  int dev = -1;
  uint64_t nw_cap = 0;
  uint64_t* d_out = nullptr;
  uint64_t* d_in = nullptr;
  uint64_t* h_out = nullptr;
  uint64_t* h_in = nullptr;

  void release()
  {
    (void)hipFree(d_out);
    (void)hipFree(d_in);
    (void)hipHostFree(h_out);
    (void)hipHostFree(h_in);
    d_out = d_in = h_out = h_in = nullptr;
    nw_cap = 0;
  }

  hipError_t reserve(uint64_t nw)
  {
    hipError_t e = hipSuccess;
    if (nw > nw_cap) {
      release();
      const size_t bytes = nw * kSlots * 8;
      if ((e = hipMalloc(&d_out, bytes)) != hipSuccess || (e = hipMalloc(&d_in, bytes)) != hipSuccess ||
          (e = hipHostMalloc(&h_out, bytes)) != hipSuccess || (e = hipHostMalloc(&h_in, bytes)) != hipSuccess) {
        release();
        return e;
      }
      nw_cap = nw;
    }
    return e;
  }
};

std::mutex g_bool_mu;
std::vector<BoolWs*> g_bool_pool;  // idle workspaces (kept for the process lifetime)

BoolWs* bool_ws_acquire(int dev)
{
  std::lock_guard<std::mutex> lk(g_bool_mu);
  for (size_t i = 0; i < g_bool_pool.size(); ++i)
    if (g_bool_pool[i]->dev == dev) {
      BoolWs* w = g_bool_pool[i];
      g_bool_pool.erase(g_bool_pool.begin() + (long)i);
      return w;
    }
  BoolWs* w = new (std::nothrow) BoolWs;
  if (w) w->dev = dev;
  return w;
}

void bool_ws_release(BoolWs* w)
{
  std::lock_guard<std::mutex> lk(g_bool_mu);
  g_bool_pool.push_back(w);
}

bool host_formula(const BoolParams& S, uint32_t bits)
{
  for (uint32_t c = 0; c < S.ncl; ++c)
    if (!((bits & S.pos[c]) | (~bits & S.neg[c]))) return false;
  return true;
}

}  // namespace

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
  const bool want = d_begin || d_end || d_lineno;
  if (want && !(d_begin && d_end && d_lineno)) return fail(UGPU_INVAL, "give all three record arrays or none");
  const bool files = (flags & UGPU_BOOL_FILES) != 0;
  if (files) used = listmask;  // every list: the whole-input literals and the lines any list touches
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint64_t per = 0, nw = 0;
  const int dev = line_wave_ranges(len, &per, &nw);
  if (dev < 0) return UGPU_DEVICE;
  BoolWs* ws = bool_ws_acquire(dev);
  if (!ws) return fail(UGPU_NOMEM, "line selection workspace");
  hipError_t e = ws->reserve(nw);
  if (e != hipSuccess) {
    bool_ws_release(ws);
    return hip_fail(e, "line selection buffers");
  }
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
  S.per = per;
  S.nwaves = nw;
  S.lastnl = ws->d_out + nw;
  S.mcover = ws->d_out + 2 * nw;
  S.selcnt = ws->d_out + kSlotLast * nw;
  S.prefix = ws->d_in;
  S.bol = ws->d_in + nw;
  S.cover = ws->d_in + 2 * nw;
  S.obase = ws->d_in + kSlotLast * nw;
  S.begin = d_begin;
  S.end = d_end;
  S.lineno = d_lineno;
  const uint64_t nsum = 2 + S.nl;  // per-wave arrays of the summary, contiguous both ways
  int rc = UGPU_OK;
  uint64_t nsel = 0;
  LinesParams L{};
  L.g = dbuf;
  L.len = len;
  L.per = per;
  L.nwaves = nw;
  L.counts = ws->d_out;
  if ((e = launch_nl_count(L, false, st)) != hipSuccess || (e = launch_bool_summary(S, st)) != hipSuccess ||
      (e = hipMemcpyAsync(ws->h_out, ws->d_out, nw * nsum * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess) {
    rc = hip_fail(e, "line summary");
  } else {
    // stitch: newlines, begin of the open line and each list's match cover before each range
    uint64_t total = 0, bol = 0, cover[UGPU_BOOL_MAX_LISTS] = {};
    for (uint64_t i = 0; i < nw; ++i) {
      ws->h_in[i] = total;
      ws->h_in[nw + i] = bol;
      total += ws->h_out[i];
      if (ws->h_out[nw + i]) bol = ws->h_out[nw + i];
      for (uint32_t t = 0; t < S.nl; ++t) {
        const uint64_t at = (2 + (uint64_t)t) * nw + i;
        ws->h_in[at] = cover[t];
        if (ws->h_out[at] > cover[t]) cover[t] = ws->h_out[at];
      }
    }
    if (lines) *lines = total + (bol < len ? 1 : 0);
    int truth = -1;
    if (files) {
      // a list with a match starting below len touches a line: the whole-input literals
      uint32_t bits = 0;
      for (uint32_t t = 0; t < S.nl; ++t)
        if (cover[t]) bits |= 1u << t;
      truth = host_formula(S, bits) ? 1 : 0;
      S.ncl = 0;
      if (truth && S.nl) {  // the lines any list touches
        S.ncl = 1;
        S.pos[0] = listmask;
        S.neg[0] = 0;
      } else {  // nothing
        S.all = 0;
        S.nl = 0;
      }
    }
    if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * nsum * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = launch_bool(S, false, st)) != hipSuccess ||
        (e = hipMemcpyAsync(ws->h_out + kSlotLast * nw, ws->d_out + kSlotLast * nw, nw * 8, hipMemcpyDeviceToHost,
                            st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess) {
      rc = hip_fail(e, "line selection count");
    } else {
      for (uint64_t i = 0; i < nw; ++i) {
        ws->h_in[kSlotLast * nw + i] = nsel;
        nsel += ws->h_out[kSlotLast * nw + i];
      }
      if (selected) *selected = nsel;
      if (whole) *whole = truth >= 0 ? truth : (nsel ? 1 : 0);
      if (want && nsel > capacity) {
        rc = fail(UGPU_CAPACITY, "line record arrays too small");
      } else if (want && nsel) {
        if ((e = hipMemcpyAsync(ws->d_in + kSlotLast * nw, ws->h_in + kSlotLast * nw, nw * 8, hipMemcpyHostToDevice,
                                st)) != hipSuccess ||
            (e = launch_bool(S, true, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
          rc = hip_fail(e, "line selection write");
      }
    }
  }
  bool_ws_release(ws);
  return rc;
}
