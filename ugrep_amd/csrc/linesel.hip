// linesel.hip -- line records on the device (the bol/eol
// half): which lines a match list selects, and the byte span of given lines.
//
// Replaces, for a fully buffered input, the per-match host walk of ugrep's
// line output (src/ugrep.cpp:11432-11521: matcher->bol() / eol(true) around
// every hit, the lines in between for -v and -A/-B/-C).
//
// Same wave-range layout as lines.hip (4 KiB tiles, tpw tiles per wave, about
// 16 waves per CU; nl_count_kernel of lines.hip supplies the per-wave newline
// counts).  A line is owned by the wave whose range holds its terminator (the
// '\n', or len for an unterminated tail: the last wave), so the records of a
// wave are contiguous and sorted and the output order is fixed by a host
// prefix of per-wave counts.
//
//   sel_summary_kernel  per wave: 1 + position of the last '\n' of its range
//                       (tiles walked from the end) and the largest
//                       exclusive end of the matches starting in the range;
//   (host)              prefix sum of the newline counts, prefix max of the
//                       other two: line number, line begin and match cover
//                       at every range start;
//   sel_kernel<false>   per wave: number of selected lines it owns;
//   (host)              exclusive prefix of those counts;
//   sel_kernel<true>    the same walk, writing (begin, end, lineno).
//   span_kernel         position of the j-th newline for an ascending list of
//                       line numbers: begin = pos(m-1)+1, end = pos(m).
//
// sel_kernel keeps, per tile, the 16-byte granule newline masks and their
// prefix in LDS (as nl_assign_kernel) plus one bit per line of the tile: the
// matches starting in the tile, 64 per step, set the bits of the lines they
// touch; `cover` (exclusive end of the bytes touched by earlier matches)
// carries a match across tiles and ranges.
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

// (tile loads, newline masks, rank_of / mark, scans, lower64: line_tiles.hpp)

// Exclusive end of the bytes match idx (start s < len) touches: a zero-length
// match touches byte s.
__device__ __forceinline__ uint64_t match_end(const SelParams& S, uint64_t idx, uint64_t s)
{
  const uint64_t l = S.lens ? (uint64_t)S.lens[idx] : 0ull;
  const uint64_t e = l ? s + l : s + 1;
  return e < S.len ? e : S.len;
}

}  // namespace

__global__ __launch_bounds__(kSWaves * 64) void sel_summary_kernel(SelParams S)
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
  const uint64_t j0 = lower64(S.starts, S.nmatch, r.lo, lane), j1 = lower64(S.starts, S.nmatch, r.hi, lane);
  uint64_t cv = 0;
  for (uint64_t idx = j0 + (uint64_t)lane; idx < j1; idx += 64) {
    const uint64_t e = match_end(S, idx, S.starts[idx]);
    cv = e > cv ? e : cv;
  }
  cv = wave_max(cv);
  if (lane == 0) {
    S.lastnl[gw] = last;
    S.mcover[gw] = cv;
  }
}

template <bool WRITE>
__global__ __launch_bounds__(kSWaves * 64) void sel_kernel(SelParams S)
{
  __shared__ uint16_t gmask[kSWaves][256], gpre[kSWaves][256];
  __shared__ uint32_t tbits[kSWaves][kTbWords];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + wid;
  if (gw >= S.nwaves) return;
  const SRange r = srange(S.len, S.per, gw);
  uint16_t* gm = gmask[wid];
  uint16_t* gp = gpre[wid];
  uint32_t* tb = tbits[wid];
  uint64_t j = lower64(S.starts, S.nmatch, r.lo, lane);  // next match to place
  uint64_t line = 1 + S.prefix[gw];                      // line of byte r.lo
  uint64_t bol = S.bol[gw];                              // begin of that line
  uint64_t cover = S.cover[gw];  // exclusive end of the bytes touched by the matches before j
  uint64_t out = WRITE ? S.obase[gw] : 0;
  uint32_t nsel = 0;             // (count pass) selected lines, per lane
  const uint32_t inv = S.invert ? 0xffffu : 0u;
  for (uint32_t i = 0; i < r.n; ++i) {
    wave_sync();  // the previous tile's LDS reads precede these writes
    const uint64_t ts = r.lo + (uint64_t)i * kSTile;
    const uint64_t tend = ts + kSTile < r.hi ? ts + kSTile : r.hi;
    uint32_t c[4];
    for (int w = lane; w < kTbWords; w += 64) tb[w] = 0;
    const uint32_t base = tile_masks(S.g, r, i, lane, gm, gp, c);
    wave_sync();
    // the open line and the lines after it that earlier matches reach
    if (cover > bol && lane == 0) {
      uint32_t hr = 0;
      if (cover > ts) hr = rank_of(gm, gp, (uint32_t)((cover < tend ? cover : tend) - 1 - ts));
      mark(tb, 0, hr);
    }
    if (j < S.nmatch) {
      uint64_t cl = 0;  // this lane's share of the tile's cover
      bool hit = false;
      for (;;) {        // matches starting in this tile, 64 at a time
        const uint64_t idx = j + (uint64_t)lane;
        const uint64_t s = idx < S.nmatch ? S.starts[idx] : ~0ull;
        const bool in = s < tend;
        const uint64_t mb = __ballot(in);
        if (!mb) break;
        hit = true;
        uint32_t r0 = 0, r1 = 0;
        if (in) {
          const uint64_t e = match_end(S, idx, s);
          cl = e > cl ? e : cl;
          r0 = rank_of(gm, gp, (uint32_t)(s - ts));
          r1 = rank_of(gm, gp, (uint32_t)((e < tend ? e : tend) - 1 - ts));
        }
        // (matches crowd on a line: one whose only line the lane below has just reached leaves the bit to it)
        const uint32_t pr1 = (uint32_t)__shfl_up((int)r1, 1, 64);
        if (in && !(lane && r0 == r1 && pr1 == r0)) mark(tb, r0, r1);
        const uint32_t k = (uint32_t)__popcll(mb);
        j += k;
        if (k < 64) break;
      }
      if (hit) {
        cl = wave_max(cl);
        cover = cl > cover ? cl : cover;
      }
    }
    wave_sync();
    // the lines ending in this tile: granule g's are ranks gp[g] .. gp[g] + c - 1
    uint32_t field[4], lp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t g = 64u * k + lane, r0 = gp[g], m = gm[g];
      const uint64_t two = (uint64_t)tb[r0 >> 5] | ((uint64_t)tb[(r0 >> 5) + 1] << 32);
      field[k] = ((uint32_t)(two >> (r0 & 31u)) ^ inv) & ((1u << c[k]) - 1u);
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
    const bool sel = (cover > bol) != (S.invert != 0);
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

__global__ __launch_bounds__(kSWaves * 64) void span_kernel(SpanParams Q)
{
  __shared__ uint16_t gmask[kSWaves][256], gpre[kSWaves][256];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + wid;
  if (gw >= Q.nwaves) return;
  const SRange r = srange(Q.len, Q.per, gw);
  uint16_t* gm = gmask[wid];
  uint16_t* gp = gpre[wid];
  const uint64_t lines = Q.newlines + (Q.len && Q.g[Q.len - 1] != '\n' ? 1 : 0);
  if (gw == 0) {  // line 0 does not exist; line 1 begins the buffer
    const uint64_t n1 = lower64(Q.q, Q.nq, 2, lane);
    for (uint64_t idx = lane; idx < n1; idx += 64) {
      if (Q.q[idx] == 0)
        Q.begin[idx] = Q.end[idx] = ~0ull;
      else if (lines)
        Q.begin[idx] = 0;
    }
  }
  if (gw == Q.nwaves - 1) {  // past the last newline: the unterminated line ends at len, others do not exist
    const uint64_t a = lower64(Q.q, Q.nq, Q.newlines + 1, lane);
    for (uint64_t idx = a + (uint64_t)lane; idx < Q.nq; idx += 64) {
      if (Q.q[idx] <= lines)
        Q.end[idx] = Q.len;
      else
        Q.begin[idx] = Q.end[idx] = ~0ull;
    }
  }
  // this wave holds the newlines of ranks (R, R + C]: the end of lines
  // R+1 .. R+C and the begin of lines R+2 .. R+C+1
  uint64_t R = Q.prefix[gw];
  const uint64_t C = Q.counts[gw], top = R + C;
  if (!C) return;
  uint64_t je = lower64(Q.q, Q.nq, R + 1, lane), jb = lower64(Q.q, Q.nq, R + 2, lane);
  if (je >= Q.nq || Q.q[je] > top + 1) return;  // no query here
  for (uint32_t i = 0; i < r.n; ++i) {
    wave_sync();
    const uint64_t ts = r.lo + (uint64_t)i * kSTile;
    uint32_t c[4];
    const uint32_t base = tile_masks(Q.g, r, i, lane, gm, gp, c);
    wave_sync();
    if (base) {
      for (;;) {  // ends: lines R+1 .. R+base
        const uint64_t idx = je + (uint64_t)lane;
        const uint64_t m = idx < Q.nq ? Q.q[idx] : ~0ull;
        const bool in = m <= R + base;
        const uint64_t mb = __ballot(in);
        if (!mb) break;
        if (in) Q.end[idx] = ts + select_nl(gm, gp, (uint32_t)(m - R));
        const uint32_t k = (uint32_t)__popcll(mb);
        je += k;
        if (k < 64) break;
      }
      for (;;) {  // begins: lines R+2 .. R+base+1
        const uint64_t idx = jb + (uint64_t)lane;
        const uint64_t m = idx < Q.nq ? Q.q[idx] : ~0ull;
        const bool in = m != ~0ull && m - 1 <= R + base;
        const uint64_t mb = __ballot(in);
        if (!mb) break;
        if (in && m <= lines) Q.begin[idx] = ts + select_nl(gm, gp, (uint32_t)(m - 1 - R)) + 1;
        const uint32_t k = (uint32_t)__popcll(mb);
        jb += k;
        if (k < 64) break;
      }
      R += base;
      if (R == top) break;
    }
    const bool more = (je < Q.nq && Q.q[je] <= top) || (jb < Q.nq && Q.q[jb] <= top + 1);
    if (!more) break;
  }
}

hipError_t launch_sel_summary(const SelParams& S, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((S.nwaves + kSWaves - 1) / kSWaves);
  hipLaunchKernelGGL(sel_summary_kernel, dim3(grid), dim3(kSWaves * 64), 0, stream, S);
  return hipGetLastError();
}

hipError_t launch_sel(const SelParams& S, bool write, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((S.nwaves + kSWaves - 1) / kSWaves);
  if (write)
    hipLaunchKernelGGL(sel_kernel<true>, dim3(grid), dim3(kSWaves * 64), 0, stream, S);
  else
    hipLaunchKernelGGL(sel_kernel<false>, dim3(grid), dim3(kSWaves * 64), 0, stream, S);
  return hipGetLastError();
}

hipError_t launch_spans(const SpanParams& Q, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((Q.nwaves + kSWaves - 1) / kSWaves);
  hipLaunchKernelGGL(span_kernel, dim3(grid), dim3(kSWaves * 64), 0, stream, Q);
  return hipGetLastError();
}

}  // namespace ugpu

// ---------------------------------------------------------------- C ABI
using namespace ugpu;

namespace {

int fail(int code, const std::string& msg) { return ugpu::host_fail(code, msg); }

int hip_fail(hipError_t e, const char* what)
{
  return ugpu::host_fail(UGPU_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// Per-call scratch, pooled per device as ugpu_lines' LinesWs (no hipMalloc or
// hipFree in a repeated call): four per-wave arrays the kernels write (newline
// counts, last newline, match cover, selected counts), the four the host
// stitches for them (newline prefix, line begin, cover, output offset) and
// pinned host copies of both.
struct SelWs {
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
      if ((e = hipMalloc(&d_out, nw * 32)) != hipSuccess || (e = hipMalloc(&d_in, nw * 32)) != hipSuccess ||
          (e = hipHostMalloc(&h_out, nw * 32)) != hipSuccess || (e = hipHostMalloc(&h_in, nw * 32)) != hipSuccess) {
        release();
        return e;
      }
      nw_cap = nw;
    }
    return e;
  }
};

std::mutex g_sel_mu;
std::vector<SelWs*> g_sel_pool;  // idle workspaces (kept for the process lifetime)

SelWs* sel_ws_acquire(int dev)
{
  std::lock_guard<std::mutex> lk(g_sel_mu);
  for (size_t i = 0; i < g_sel_pool.size(); ++i)
    if (g_sel_pool[i]->dev == dev) {
      SelWs* w = g_sel_pool[i];
      g_sel_pool.erase(g_sel_pool.begin() + (long)i);
      return w;
    }
  SelWs* w = new (std::nothrow) SelWs;
  if (w) w->dev = dev;
  return w;
}

void sel_ws_release(SelWs* w)
{
  std::lock_guard<std::mutex> lk(g_sel_mu);
  g_sel_pool.push_back(w);
}

// wave ranges as ugpu_lines': whole tiles, about 16 waves per CU, at most kMaxRec
int wave_ranges(uint64_t len, uint64_t* per, uint64_t* nwaves)
{
  int dev = 0, cus = 256;
  hipError_t e;
  if ((e = hipGetDevice(&dev)) != hipSuccess ||
      (e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) {
    hip_fail(e, "device query");
    return -1;
  }
  const uint64_t tile = lines_tile();
  const uint64_t tiles = (len + tile - 1) / tile;
  uint64_t want = (uint64_t)cus * 16;
  if (want > (uint64_t)kMaxRec) want = kMaxRec;
  uint64_t tpw = tiles ? (tiles + want - 1) / want : 1;
  while (tpw * tile > kMaxRecBytes) --tpw;
  if (tpw == 0) tpw = 1;
  *per = tpw * tile;
  *nwaves = tiles ? (tiles + tpw - 1) / tpw : 1;
  return dev;
}

// nl_count_kernel into ws->d_out[0, nw); leaves the launch on the stream
hipError_t count_newlines(SelWs* ws, const uint8_t* dbuf, uint64_t len, uint64_t per, uint64_t nw, hipStream_t st)
{
  LinesParams L{};
  L.g = dbuf;
  L.len = len;
  L.per = per;
  L.nwaves = nw;
  L.counts = ws->d_out;
  return launch_nl_count(L, false, st);
}

}  // namespace

int ugpu::line_wave_ranges(uint64_t len, uint64_t* per, uint64_t* nwaves) { return wave_ranges(len, per, nwaves); }

int ugpu_select_lines(const uint8_t* dbuf, uint64_t len, const uint64_t* d_start, const uint32_t* d_len, uint64_t n,
                      uint32_t flags, uint64_t* d_begin, uint64_t* d_end, uint64_t* d_lineno, uint64_t capacity,
                      uint64_t* selected, uint64_t* lines, void* stream)
{
  if (!dbuf || (n && !d_start)) return fail(UGPU_INVAL, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dbuf) & 15u) return fail(UGPU_INVAL, "buffer must be 16-byte aligned");
  if (flags & ~UGPU_SEL_INVERT) return fail(UGPU_INVAL, "unknown flags");
  const bool want = d_begin || d_end || d_lineno;
  if (want && !(d_begin && d_end && d_lineno)) return fail(UGPU_INVAL, "give all three record arrays or none");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint64_t per = 0, nw = 0;
  const int dev = wave_ranges(len, &per, &nw);
  if (dev < 0) return UGPU_DEVICE;
  SelWs* ws = sel_ws_acquire(dev);
  if (!ws) return fail(UGPU_NOMEM, "line selection workspace");
  hipError_t e = ws->reserve(nw);
  if (e != hipSuccess) {
    sel_ws_release(ws);
    return hip_fail(e, "line selection buffers");
  }
  SelParams S{};
  S.g = dbuf;
  S.len = len;
  S.per = per;
  S.nwaves = nw;
  S.starts = d_start;
  S.lens = d_len;
  S.nmatch = n;
  S.invert = flags & UGPU_SEL_INVERT;
  S.lastnl = ws->d_out + nw;
  S.mcover = ws->d_out + 2 * nw;
  S.selcnt = ws->d_out + 3 * nw;
  S.prefix = ws->d_in;
  S.bol = ws->d_in + nw;
  S.cover = ws->d_in + 2 * nw;
  S.obase = ws->d_in + 3 * nw;
  S.begin = d_begin;
  S.end = d_end;
  S.lineno = d_lineno;
  int rc = UGPU_OK;
  uint64_t nsel = 0;
  if ((e = count_newlines(ws, dbuf, len, per, nw, st)) != hipSuccess ||
      (e = launch_sel_summary(S, st)) != hipSuccess ||
      (e = hipMemcpyAsync(ws->h_out, ws->d_out, nw * 24, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess) {
    rc = hip_fail(e, "line summary");
  } else {
    // stitch: newlines, begin of the open line and match cover before each range
    uint64_t total = 0, bol = 0, cover = 0;
    for (uint64_t i = 0; i < nw; ++i) {
      ws->h_in[i] = total;
      ws->h_in[nw + i] = bol;
      ws->h_in[2 * nw + i] = cover;
      total += ws->h_out[i];
      if (ws->h_out[nw + i]) bol = ws->h_out[nw + i];
      if (ws->h_out[2 * nw + i] > cover) cover = ws->h_out[2 * nw + i];
    }
    if (lines) *lines = total + (bol < len ? 1 : 0);
    if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * 24, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = launch_sel(S, false, st)) != hipSuccess ||
        (e = hipMemcpyAsync(ws->h_out + 3 * nw, ws->d_out + 3 * nw, nw * 8, hipMemcpyDeviceToHost, st)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess) {
      rc = hip_fail(e, "line selection count");
    } else {
      for (uint64_t i = 0; i < nw; ++i) {
        ws->h_in[3 * nw + i] = nsel;
        nsel += ws->h_out[3 * nw + i];
      }
      if (selected) *selected = nsel;
      if (want && nsel > capacity) {
        rc = fail(UGPU_CAPACITY, "line record arrays too small");
      } else if (want && nsel) {
        if ((e = hipMemcpyAsync(ws->d_in + 3 * nw, ws->h_in + 3 * nw, nw * 8, hipMemcpyHostToDevice, st)) !=
                hipSuccess ||
            (e = launch_sel(S, true, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
          rc = hip_fail(e, "line selection write");
      }
    }
  }
  sel_ws_release(ws);
  return rc;
}

int ugpu_line_spans(const uint8_t* dbuf, uint64_t len, const uint64_t* d_lineno, uint64_t n, uint64_t* d_begin,
                    uint64_t* d_end, void* stream)
{
  if (!dbuf || (n && !(d_lineno && d_begin && d_end))) return fail(UGPU_INVAL, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dbuf) & 15u) return fail(UGPU_INVAL, "buffer must be 16-byte aligned");
  if (!n) return UGPU_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint64_t per = 0, nw = 0;
  const int dev = wave_ranges(len, &per, &nw);
  if (dev < 0) return UGPU_DEVICE;
  SelWs* ws = sel_ws_acquire(dev);
  if (!ws) return fail(UGPU_NOMEM, "line span workspace");
  hipError_t e = ws->reserve(nw);
  if (e != hipSuccess) {
    sel_ws_release(ws);
    return hip_fail(e, "line span buffers");
  }
  int rc = UGPU_OK;
  if ((e = count_newlines(ws, dbuf, len, per, nw, st)) != hipSuccess ||
      (e = hipMemcpyAsync(ws->h_out, ws->d_out, nw * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess) {
    rc = hip_fail(e, "newline count");
  } else {
    uint64_t total = 0;
    for (uint64_t i = 0; i < nw; ++i) {
      ws->h_in[i] = total;
      total += ws->h_out[i];
    }
    SpanParams Q{};
    Q.g = dbuf;
    Q.len = len;
    Q.per = per;
    Q.nwaves = nw;
    Q.q = d_lineno;
    Q.nq = n;
    Q.counts = ws->d_out;
    Q.prefix = ws->d_in;
    Q.newlines = total;
    Q.begin = d_begin;
    Q.end = d_end;
    if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = launch_spans(Q, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
      rc = hip_fail(e, "line spans");
  }
  sel_ws_release(ws);
  return rc;
}
