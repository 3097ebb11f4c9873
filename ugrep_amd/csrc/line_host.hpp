// line_host.hpp -- the host layer of the line calls (lines.hip, linesel.hip,
// linebool.hip, batch.hip): the wave ranges, the per-wave workspace, the
// newline count with its prefix, and the driver of the two selection calls.
// Error reporting, the buffers and the workspace pool come from hip_host.hpp.
#pragma once
#include "hip_host.hpp"
#include "scan_kernels.hpp"

namespace ugpu {

// The wave ranges of the line kernels for a buffer of len bytes: whole tiles,
// about 16 waves per CU, at most kMaxRec.  Returns the current device, or -1
// with the error recorded.
inline int line_wave_ranges(uint64_t len, uint64_t* per, uint64_t* nwaves)
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
  while (tpw * tile > kMaxRecBytes) --tpw;  // (never for sane sizes; 32-bit offsets)
  if (tpw == 0) tpw = 1;
  *per = tpw * tile;
  *nwaves = tiles ? (tiles + tpw - 1) / tpw : 1;
  return dev;
}

// `slots` per-wave uint64_t arrays the kernels write (d_out: array s is
// d_out + s * nw), as many the host stitches for them (d_in), and pinned host
// copies of both.  Grows only.
struct WaveWs {
  int dev = -1;
  DevBuf<uint64_t> d_out, d_in;
  PinBuf<uint64_t> h_out, h_in;

  void release()
  {
    d_out.release();
    d_in.release();
    h_out.release();
    h_in.release();
  }

  hipError_t reserve(uint64_t nw, uint64_t slots)
  {
    const uint64_t n = nw * slots;
    if (n <= h_in.cap) return hipSuccess;  // (the last of the four: all have room)
    release();
    hipError_t e;
    if ((e = d_out.alloc(n)) != hipSuccess || (e = d_in.alloc(n)) != hipSuccess || (e = h_out.alloc(n)) != hipSuccess ||
        (e = h_in.alloc(n)) != hipSuccess)
      release();
    return e;
  }
};

// nl_count_kernel over L's wave ranges into array 0 of ws.d_out, then `also`
// (further launches writing arrays 1 .. back-1); the `back` arrays are copied to
// ws.h_out and the stream is synchronised.  Leaves the exclusive prefix of the
// newline counts in array 0 of ws.h_in and their sum in *newlines.
template <class Also>
hipError_t newline_prefix(WaveWs& ws, LinesParams L, bool sparse, uint64_t back, Also also, hipStream_t st,
                          uint64_t* newlines)
{
  L.counts = ws.d_out;
  hipError_t e;
  if ((e = launch_nl_count(L, sparse, st)) != hipSuccess || (e = also()) != hipSuccess ||
      (e = hipMemcpyAsync(ws.h_out, ws.d_out, L.nwaves * back * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)
    return e;
  uint64_t total = 0;
  for (uint64_t i = 0; i < L.nwaves; ++i) {
    ws.h_in[i] = total;
    total += ws.h_out[i];
  }
  *newlines = total;
  return hipSuccess;
}

inline hipError_t newline_prefix(WaveWs& ws, const LinesParams& L, bool sparse, hipStream_t st, uint64_t* newlines)
{
  return newline_prefix(ws, L, sparse, 1, [] { return hipSuccess; }, st, newlines);
}

// The stitch of ugpu_columns.  out: the summary pass's four per-range arrays
// (newlines, 1 + last newline, column function a | kind << 32, b: ColParams);
// in: what holds at each range's first byte (newlines before it, begin of its
// line, its column).  A line may run through many ranges, and one of 4 GiB or
// more has columns past 2^32: everything is 64 bits here.
inline void column_stitch(const uint64_t* out, uint64_t* in, uint64_t nw, uint32_t tmask)
{
  uint64_t newlines = 0, bol = 0, k = 0;
  for (uint64_t i = 0; i < nw; ++i) {
    in[i] = newlines;
    in[nw + i] = bol;
    in[2 * nw + i] = k;
    newlines += out[i];
    if (out[nw + i]) bol = out[nw + i];
    const uint64_t a = out[2 * nw + i] & 0xffffffffu, b = out[3 * nw + i];
    switch ((uint32_t)(out[2 * nw + i] >> 32)) {
      case kColAdd: k += a; break;
      case kColTab: k = ((k + a) | tmask) + 1 + b; break;
      default: k = a; break;
    }
  }
}

// The stitch of ugpu_transcode.  out: the summary pass's three per-range arrays
// (output bytes for the incoming bit 0, for the incoming bit 1, the range
// function: TcParams; without `carry` only the first is read); in: each
// range's exclusive output offset and its incoming bit.  Returns the output
// length; an output passes 4 GiB from 2 GiB of Latin-1.
inline uint64_t transcode_stitch(const uint64_t* out, uint64_t* in, uint64_t nw, bool carry)
{
  uint64_t off = 0, c = 0;
  for (uint64_t i = 0; i < nw; ++i) {
    in[i] = off;
    in[nw + i] = c;
    off += out[(c ? nw : 0) + i];
    if (carry) c = (out[2 * nw + i] >> c) & 1u;
  }
  return off;
}

inline LinesParams line_ranges_params(const uint8_t* g, uint64_t len, uint64_t per, uint64_t nw)
{
  LinesParams L{};
  L.g = g;
  L.len = len;
  L.per = per;
  L.nwaves = nw;
  return L;
}

// The selection call over ncover match lists (ugpu_select_lines: 1;
// ugpu_select_lines_bool: the lists its formula uses).  c holds the buffer,
// invert and the record arrays; the driver sets the wave ranges and the
// per-wave arrays, laid out as: newline counts / prefix, last newline / line
// begin, ncover covers, selected counts / output offsets.  Three host round
// trips, two when it only counts:
//   newline count and summary(); the stitch: prefix sum of the counts, prefix
//   maxima of the others; decide(final covers) may then change the pass's
//   parameters and returns the whole-input truth, or -1 for "some line is
//   selected";
//   pass(false), the count pass; the exclusive prefix of its counts; *selected,
//   *whole and the capacity check;
//   pass(true), the write pass.
template <class P, class Summary, class Decide, class Pass>
int select_lines_driver(P& c, uint32_t ncover, uint64_t capacity, uint64_t* selected, uint64_t* lines,
                        int* whole, hipStream_t st, Summary summary, Decide decide, Pass pass)
{
  const bool want = c.begin || c.end || c.lineno;
  if (want && !(c.begin && c.end && c.lineno)) return fail(UGPU_INVAL, "give all three record arrays or none");
  const int dev = line_wave_ranges(c.len, &c.per, &c.nwaves);
  if (dev < 0) return UGPU_DEVICE;
  WsLease<WaveWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "line selection workspace");
  const uint64_t nw = c.nwaves, nsum = 2 + ncover, last = nsum * nw;  // last: the selected counts
  hipError_t e = ws->reserve(nw, nsum + 1);
  if (e != hipSuccess) return hip_fail(e, "line selection buffers");
  c.lastnl = ws->d_out + nw;
  c.mcover = ws->d_out + 2 * nw;
  c.selcnt = ws->d_out + last;
  c.prefix = ws->d_in;
  c.bol = ws->d_in + nw;
  c.cover = ws->d_in + 2 * nw;
  c.obase = ws->d_in + last;
  uint64_t total = 0;
  if ((e = newline_prefix(*ws.ws, line_ranges_params(c.g, c.len, c.per, nw), false, nsum, summary, st, &total)) !=
      hipSuccess)
    return hip_fail(e, "line summary");
  // stitch: begin of the open line and each list's match cover before each range
  uint64_t bol = 0, cover[kBoolLists] = {};
  for (uint64_t i = 0; i < nw; ++i) {
    ws->h_in[nw + i] = bol;
    if (ws->h_out[nw + i]) bol = ws->h_out[nw + i];
    for (uint32_t t = 0; t < ncover; ++t) {
      const uint64_t at = (2 + (uint64_t)t) * nw + i;
      ws->h_in[at] = cover[t];
      if (ws->h_out[at] > cover[t]) cover[t] = ws->h_out[at];
    }
  }
  if (lines) *lines = total + (bol < c.len ? 1 : 0);
  const int truth = decide(cover);
  if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * nsum * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = pass(false)) != hipSuccess ||
      (e = hipMemcpyAsync(ws->h_out + last, ws->d_out + last, nw * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "line selection count");
  uint64_t nsel = 0;
  for (uint64_t i = 0; i < nw; ++i) {
    ws->h_in[last + i] = nsel;
    nsel += ws->h_out[last + i];
  }
  if (selected) *selected = nsel;
  if (whole) *whole = truth >= 0 ? truth : (nsel ? 1 : 0);
  if (want && nsel > capacity) return fail(UGPU_CAPACITY, "line record arrays too small");
  if (want && nsel) {
    if ((e = hipMemcpyAsync(ws->d_in + last, ws->h_in + last, nw * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = pass(true)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
      return hip_fail(e, "line selection write");
  }
  return UGPU_OK;
}

}  // namespace ugpu
