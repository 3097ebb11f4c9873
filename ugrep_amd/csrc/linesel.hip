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
#include "device_common.hpp"
#include "line_host.hpp"
#include "line_select.hpp"

namespace ugpu {

// (tiles, masks, rank_of / mark, scans, lower64: line_tiles.hpp; the steps of
// the walk shared with bool_kernel: line_select.hpp)

__global__ __launch_bounds__(kSWaves * 64) void sel_summary_kernel(SelParams S)
{
  const int lane = threadIdx.x & 63;
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (gw >= S.nwaves) return;
  const SRange r = srange(S.len, S.per, gw);
  const uint64_t last = last_newline(S.g, r, lane);
  const uint64_t cv = range_cover(S.starts, S.lens, S.nmatch, S.len, r, lane);
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
    mark_cover(tb, gm, gp, cover, bol, ts, tend, lane);
    if (j < S.nmatch) {
      uint64_t cl;
      const uint64_t j1 = place_matches(tb, gm, gp, S.starts, S.lens, S.nmatch, S.len, j, ts, tend, lane, cl);
      if (j1 != j) {
        cl = wave_max(cl);
        cover = cl > cover ? cl : cover;
        j = j1;
      }
    }
    wave_sync();
    // the lines ending in this tile, per granule: their bits and 1 + tile offset of its last newline
    uint32_t field[4], lp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t g = 64u * k + lane;
      field[k] = granule_field(tb, gp[g], c[k], inv);
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
  if (gw == S.nwaves - 1 && bol < S.len && (cover > bol) != (S.invert != 0))  // the unterminated last line
    tail_line<WRITE>(bol, S.len, line, out, lane, S.begin, S.end, S.lineno, total);
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

int ugpu_select_lines(const uint8_t* dbuf, uint64_t len, const uint64_t* d_start, const uint32_t* d_len, uint64_t n,
                      uint32_t flags, uint64_t* d_begin, uint64_t* d_end, uint64_t* d_lineno, uint64_t capacity,
                      uint64_t* selected, uint64_t* lines, void* stream)
{
  if (!dbuf || (n && !d_start)) return fail(UGPU_INVAL, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dbuf) & 15u) return fail(UGPU_INVAL, "buffer must be 16-byte aligned");
  if (flags & ~UGPU_SEL_INVERT) return fail(UGPU_INVAL, "unknown flags");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SelParams S{};
  S.g = dbuf;
  S.len = len;
  S.invert = flags & UGPU_SEL_INVERT;
  S.begin = d_begin;
  S.end = d_end;
  S.lineno = d_lineno;
  S.starts = d_start;
  S.lens = d_len;
  S.nmatch = n;
  return select_lines_driver(
      S, 1, capacity, selected, lines, nullptr, st, [&] { return launch_sel_summary(S, st); },
      [](const uint64_t*) { return -1; }, [&](bool write) { return launch_sel(S, write, st); });
}

int ugpu_line_spans(const uint8_t* dbuf, uint64_t len, const uint64_t* d_lineno, uint64_t n, uint64_t* d_begin,
                    uint64_t* d_end, void* stream)
{
  if (!dbuf || (n && !(d_lineno && d_begin && d_end))) return fail(UGPU_INVAL, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dbuf) & 15u) return fail(UGPU_INVAL, "buffer must be 16-byte aligned");
  if (!n) return UGPU_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint64_t per = 0, nw = 0;
  const int dev = line_wave_ranges(len, &per, &nw);
  if (dev < 0) return UGPU_DEVICE;
  WsLease<WaveWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "line span workspace");
  hipError_t e = ws->reserve(nw, 1);
  if (e != hipSuccess) return hip_fail(e, "line span buffers");
  SpanParams Q{};
  if ((e = newline_prefix(*ws.ws, line_ranges_params(dbuf, len, per, nw), false, st, &Q.newlines)) != hipSuccess)
    return hip_fail(e, "newline count");
  Q.g = dbuf;
  Q.len = len;
  Q.per = per;
  Q.nwaves = nw;
  Q.q = d_lineno;
  Q.nq = n;
  Q.counts = ws->d_out;
  Q.prefix = ws->d_in;
  Q.begin = d_begin;
  Q.end = d_end;
  if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = launch_spans(Q, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "line spans");
  return UGPU_OK;
}
