// batch.hip -- per-input records of a batched FIND.
//
// ugpu_find_batch (engine.hip) packs many inputs into one buffer, each ended
// by '\n', and scans the packed buffer once.  Replaces ugrep's per-file loop
// (src/ugrep.cpp:4261-4480, one job per file, each with its own matcher pass,
// line counter and totals) for the part after the scan: the packed match list
// is cut at the inputs' bounds into what grep reports per file.
//
// ugpu_split_matches, over the sorted match list and the nseg + 1 ascending
// bounds:
//   nl_count_kernel      (lines.hip) newlines per wave range; the host makes
//                        their exclusive prefix, as ugpu_lines does;
//   split_walk_kernel    the tile walk of nl_assign_kernel over two sorted
//                        position lists at once, the match starts and the
//                        bounds: the packed line of each, one read of the
//                        buffer for both;
//   split_bounds_kernel  one thread per bound: first[s] (binary search of the
//                        match list), newlines[s] from the bounds' lines, and
//                        the zeroes of the three sums;
//   split_records_kernel one thread per record: its segment (binary search of
//                        the bounds), rel, line, and the integer sums digest,
//                        dcap and mlines -- combined inside the wave per run
//                        of equal segments (records are sorted, so a segment
//                        is a run of lanes), one 64-bit vector atomic add per
//                        run and sum.  Integer sums mod 2^64 do not depend on
//                        the order of the adds: results repeat exactly.
#include "device_common.hpp"
#include "line_host.hpp"
#include "line_tiles.hpp"

namespace ugpu {

namespace {

struct SplitParams {
  const uint8_t* g;  // 16-byte aligned buffer
  uint64_t len, per, nwaves;
  const uint64_t* prefix;  // newlines before each wave range
  uint64_t total;          // newlines of the buffer
  const uint64_t* starts;
  const uint32_t* lens;    // or NULL: 0
  const uint32_t* caps;    // or NULL: cap1
  uint32_t cap1;
  uint64_t n;
  const uint64_t* bounds;
  uint64_t nb;             // nseg + 1
  uint64_t* sline;         // n: packed line of each start below len
  uint64_t* bline;         // nb: packed line of each bound below len
  uint64_t *first, *digest, *dcap, *newlines, *mlines, *rel, *line;
};

constexpr int kSplitThreads = 256;

// The entries of the sorted list a[j..) below tend, 64 at a time: out[idx] =
// the line of the tile's first byte + the entry's rank in the tile.  Entries
// below the tile's begin ts were consumed by the tiles before.
__device__ __forceinline__ void walk_list(const uint64_t* a, uint64_t na, uint64_t& j, uint64_t ts, uint64_t tend,
                                          uint64_t line, const uint16_t* gm, const uint16_t* gp, uint64_t* out,
                                          int lane)
{
  for (;;) {
    const uint64_t idx = j + (uint64_t)lane;
    const uint64_t s = idx < na ? a[idx] : ~0ull;
    const bool in = s < tend;
    const uint64_t mb = __ballot(in);
    if (!mb) break;
    if (in) out[idx] = line + rank_of(gm, gp, (uint32_t)(s - ts));
    const uint32_t k = (uint32_t)__popcll(mb);
    j += k;
    if (k < 64) break;
  }
}

__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, int lane)
{
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// number of entries of the sorted list a[0, n) that are < key (upper = false)
// or <= key (upper = true)
__device__ __forceinline__ uint64_t bsearch64(const uint64_t* a, uint64_t n, uint64_t key, bool upper)
{
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint64_t v = a[mid];
    if (upper ? v <= key : v < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// packed line of bound x: a bound at len lies after every newline
__device__ __forceinline__ uint64_t bound_line(const SplitParams& S, uint64_t x)
{
  return S.bounds[x] >= S.len ? S.total + 1 : S.bline[x];
}

}  // namespace

__global__ __launch_bounds__(kSWaves * 64) void split_walk_kernel(SplitParams S)
{
  __shared__ uint16_t gmask[kSWaves][256], gpre[kSWaves][256];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + wid;
  if (gw >= S.nwaves) return;
  const SRange r = srange(S.len, S.per, gw);
  uint64_t ja = lower64(S.starts, S.n, r.lo, lane);
  uint64_t jb = lower64(S.bounds, S.nb, r.lo, lane);
  uint64_t line = 1 + S.prefix[gw];  // line of byte r.lo
  uint16_t* gm = gmask[wid];
  uint16_t* gp = gpre[wid];
  for (uint32_t i = 0; i < r.n; ++i) {
    const bool more_a = ja < S.n && S.starts[ja] < r.hi;
    const bool more_b = jb < S.nb && S.bounds[jb] < r.hi;
    if (!more_a && !more_b) break;  // neither list has a further entry in this range
    wave_sync();  // the previous tile's LDS reads precede these writes
    const uint64_t ts = r.lo + (uint64_t)i * kSTile;
    uint32_t c[4];
    const uint32_t base = tile_masks(S.g, r, i, lane, gm, gp, c);
    wave_sync();
    const uint64_t tend = ts + kSTile < r.hi ? ts + kSTile : r.hi;
    walk_list(S.starts, S.n, ja, ts, tend, line, gm, gp, S.sline, lane);
    walk_list(S.bounds, S.nb, jb, ts, tend, line, gm, gp, S.bline, lane);
    line += base;
  }
}

__global__ __launch_bounds__(kSplitThreads) void split_bounds_kernel(SplitParams S)
{
  const uint64_t s = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
  if (s >= S.nb) return;
  S.first[s] = bsearch64(S.starts, S.n, S.bounds[s], false);
  if (s + 1 < S.nb) {
    S.newlines[s] = bound_line(S, s + 1) - bound_line(S, s);
    S.digest[s] = 0;
    S.dcap[s] = 0;
    S.mlines[s] = 0;
  }
}

__global__ __launch_bounds__(kSplitThreads) void split_records_kernel(SplitParams S)
{
  const int lane = threadIdx.x & 63;
  const uint64_t idx = (uint64_t)blockIdx.x * kSplitThreads + threadIdx.x;
  const uint64_t nseg = S.nb - 1;
  // the record's segment: the last bound at or below its start (no lane leaves
  // before the wave's shuffles)
  uint64_t seg = ~0ull, dg = 0, dc = 0;
  uint32_t ml = 0;
  if (idx < S.n) {
    const uint64_t st = S.starts[idx];
    const uint64_t ub = bsearch64(S.bounds, S.nb, st, true);
    uint64_t rel = 0, ln = 0;
    if (ub > 0 && ub - 1 < nseg) {
      seg = ub - 1;
      const uint64_t b = S.bounds[seg];
      const uint64_t sl = S.sline[idx];
      rel = st - b;
      ln = sl - bound_line(S, seg) + 1;
      dg = rel * 31u + (S.lens ? S.lens[idx] : 0u);
      dc = (rel + 1) * (uint64_t)(S.caps ? S.caps[idx] : S.cap1);
      // the first record of its line within the segment
      ml = idx == 0 || S.starts[idx - 1] < b || S.sline[idx - 1] != sl ? 1u : 0u;
    }
    if (S.rel) S.rel[idx] = rel;
    if (S.line) S.line[idx] = ln;
  }
  // sums per run of equal segments: inclusive scans, the run's sum is the
  // difference between its last lane and the lane before its first
  const uint64_t prev = __shfl_up(seg, 1, 64), next = __shfl_down(seg, 1, 64);
  const bool head = lane == 0 || prev != seg;
  const bool tail = lane == 63 || next != seg;
  const uint64_t heads = __ballot(head);
  const int firstl = 63 - __clzll((long long)(heads & lowbits((uint64_t)lane + 1)));
  const uint64_t idg = wave_scan64(dg, lane), idc = wave_scan64(dc, lane);
  const uint32_t iml = lscan_add(ml);
  const uint64_t bdg = __shfl(idg - dg, firstl, 64), bdc = __shfl(idc - dc, firstl, 64);
  const uint32_t bml = (uint32_t)__shfl((int)(iml - ml), firstl, 64);
  if (tail && seg != ~0ull) {
    atomicAdd(reinterpret_cast<unsigned long long*>(S.digest + seg), (unsigned long long)(idg - bdg));
    atomicAdd(reinterpret_cast<unsigned long long*>(S.dcap + seg), (unsigned long long)(idc - bdc));
    if (iml != bml) atomicAdd(reinterpret_cast<unsigned long long*>(S.mlines + seg), (unsigned long long)(iml - bml));
  }
}

}  // namespace ugpu

// ---------------------------------------------------------------- C ABI
using namespace ugpu;

namespace {

// Per-call scratch beside the per-wave counts and prefixes: the packed lines
// of the starts and of the bounds.
struct SplitWs : WaveWs {
  DevBuf<uint64_t> d_ln;

  hipError_t reserve_lines(uint64_t k) { return d_ln.reserve(k, k + k / 4); }
};

}  // namespace

int ugpu_split_matches(const uint8_t* dbuf, uint64_t len, const uint64_t* d_bounds, uint32_t nseg,
                       const uint64_t* d_start, const uint32_t* d_len, const uint32_t* d_cap, uint32_t cap1, uint64_t n,
                       uint64_t* d_first, uint64_t* d_digest, uint64_t* d_dcap, uint64_t* d_newlines,
                       uint64_t* d_mlines, uint64_t* d_rel, uint64_t* d_line, void* stream)
{
  if (!dbuf || !d_bounds || !d_first || (n && !d_start)) return fail(UGPU_INVAL, "NULL argument");
  if (nseg && (!d_digest || !d_dcap || !d_newlines || !d_mlines)) return fail(UGPU_INVAL, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dbuf) & 15u) return fail(UGPU_INVAL, "buffer must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint64_t per = 0, nw = 0;
  const int dev = line_wave_ranges(len, &per, &nw);
  if (dev < 0) return UGPU_DEVICE;
  WsLease<SplitWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "split workspace");
  const uint64_t nb = (uint64_t)nseg + 1;
  hipError_t e = ws->reserve(nw, 1);
  if (e == hipSuccess) e = ws->reserve_lines(n + nb);
  if (e != hipSuccess) return hip_fail(e, "split buffers");
  const LinesParams L = line_ranges_params(dbuf, len, per, nw);
  uint64_t total = 0;
  if ((e = newline_prefix(*ws.ws, L, false, st, &total)) != hipSuccess) return hip_fail(e, "newline count");
  SplitParams S{};
  S.g = dbuf;
  S.len = len;
  S.per = per;
  S.nwaves = nw;
  S.prefix = ws->d_in;
  S.total = total;
  S.starts = d_start;
  S.lens = d_len;
  S.caps = d_cap;
  S.cap1 = cap1;
  S.n = n;
  S.bounds = d_bounds;
  S.nb = nb;
  S.sline = ws->d_ln;
  S.bline = ws->d_ln + n;
  S.first = d_first;
  S.digest = d_digest;
  S.dcap = d_dcap;
  S.newlines = d_newlines;
  S.mlines = d_mlines;
  S.rel = d_rel;
  S.line = d_line;
  if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * 8, hipMemcpyHostToDevice, st)) != hipSuccess)
    return hip_fail(e, "newline prefix");
  hipLaunchKernelGGL(split_walk_kernel, dim3((uint32_t)((nw + kSWaves - 1) / kSWaves)), dim3(kSWaves * 64), 0, st, S);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "split walk");
  hipLaunchKernelGGL(split_bounds_kernel, dim3((uint32_t)((nb + kSplitThreads - 1) / kSplitThreads)),
                     dim3(kSplitThreads), 0, st, S);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "split bounds");
  if (n) {
    const uint64_t blocks = (n + kSplitThreads - 1) / kSplitThreads;
    if (blocks > 0x7fffffffull) return fail(UGPU_INVAL, "too many records");
    hipLaunchKernelGGL(split_records_kernel, dim3((uint32_t)blocks), dim3(kSplitThreads), 0, st, S);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "split records");
  }
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "split");
  return UGPU_OK;
}
