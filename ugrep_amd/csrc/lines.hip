// lines.hip -- line-level consumers of the FIND results.
//
// Replaces, for a fully buffered input:
//   * newline counting for line numbers: AbstractMatcher::lineno()
//     (include/reflex/absmatcher.h:695-766) over simd nlcount
//     (lib/simd.cpp:62-166, lib/simd_avx2.cpp:48-79);
//   * ugrep -c's matching-line count: one count per line holding a match, the
//     search skipping to the next line after the first hit
//     (src/ugrep.cpp:10567-10586).  For patterns whose matches cannot contain
//     '\n' this is the number of distinct lines holding a match start.
//
// Two wave-persistent passes over 4 KiB tiles (the sparse kernel's load
// scheme: per-tile buffer resources, non-temporal 16 B/lane loads):
//   nl_count_kernel  newlines per wave range (sparse mode: also per 1 KiB
//                    quarter, u16, 1/512 of the input written);
//   (host)           exclusive scan of the per-wave counts (<= 8192 values);
//   nl_assign_kernel line = 1 + newlines before each match start, walking the
//                    sorted match list alongside the bytes, 64 matches per
//                    step; per-wave line transition counts for -c, stitched on
//                    the host.  Dense mode reloads every tile and keeps its
//                    16-byte granule masks and prefix in LDS; sparse mode
//                    (matches rarer than one per ~2 KiB, e.g. C2) loads only
//                    the quarters holding a match start, adds the quarter
//                    prefix from qcount and gathers granule masks across lanes
//                    with ds_bpermute, so the second pass reads ~1 KiB per
//                    match instead of the whole buffer.
#include "device_common.hpp"
#include "line_host.hpp"
#include "line_tiles.hpp"

namespace ugpu {

namespace {

// (tile loads, newline masks, scans, srange, lower64, tile_masks: line_tiles.hpp)

// Per-wave -c bookkeeping over the wave's matches in order, 64 at a time
// (lanes holding a match form a prefix).
struct LineStats {
  uint64_t prev_line = 0, first_line = 0, trans = 0, nm = 0;

  __device__ __forceinline__ void add(uint64_t ln, bool in, uint64_t mb, int lane)
  {
    const uint64_t pl = __shfl_up(ln, 1, 64);
    const uint64_t before = lane == 0 ? prev_line : pl;
    const bool newl = in && (nm + (uint64_t)lane == 0 || ln != before);
    const uint32_t k = (uint32_t)__popcll(mb);
    trans += __popcll(__ballot(newl));
    if (nm == 0) first_line = __shfl(ln, 0, 64);
    prev_line = __shfl(ln, (int)k - 1, 64);
    nm += k;
  }

  __device__ __forceinline__ void store(LineRec* rec, int lane) const
  {
    if (lane == 0) {
      LineRec r;
      r.first_line = first_line;
      r.last_line = prev_line;
      r.trans = trans;
      r.nmatch = nm;
      *rec = r;
    }
  }
};

}  // namespace

template <bool SPARSE>
__global__ __launch_bounds__(kSWaves * 64) void nl_count_kernel(LinesParams L)
{
  const int lane = threadIdx.x & 63;
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (gw >= L.nwaves) return;
  const SRange r = srange(L.len, L.per, gw);
  uint32_t cnt = 0;
  for (uint32_t i = 0; i < r.n; ++i) {
    const __amdgpu_buffer_rsrc_t rs = ltile(L.g + r.lo, i, r.rel16);
    uint32_t c[4];
    if ((i + 1u) * (uint32_t)kSTile <= r.rel) {  // whole tile (uniform branch)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint4 v = sload16(rs, 16u * lane + 1024u * k);
        c[k] = __popc(nl_bits(v.x)) + __popc(nl_bits(v.y)) + __popc(nl_bits(v.z)) + __popc(nl_bits(v.w));
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t o = 16u * lane + 1024u * k;
        c[k] = __popc(nl16(sload16(rs, o)) & granule_valid(r.rel, i * (uint32_t)kSTile + o));
      }
    }
    cnt += c[0] + c[1] + c[2] + c[3];
    if (SPARSE) {  // quarter counts (<= 1024 each) packed two per dword, one scan each
      const uint32_t p01 = (uint32_t)__builtin_amdgcn_readlane(lscan_add(c[0] | (c[1] << 16)), 63);
      const uint32_t p23 = (uint32_t)__builtin_amdgcn_readlane(lscan_add(c[2] | (c[3] << 16)), 63);
      if (lane == 0)
        reinterpret_cast<uint64_t*>(L.qcount)[(r.lo / kSTile) + i] = (uint64_t)p01 | ((uint64_t)p23 << 32);
    }
  }
  const uint64_t t = wave_sum(cnt);
  if (lane == 0) L.counts[gw] = t;
}

__global__ __launch_bounds__(kSWaves * 64) void nl_assign_kernel(LinesParams L)
{
  __shared__ uint16_t gmask[kSWaves][256], gpre[kSWaves][256];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + wid;
  if (gw >= L.nwaves) return;
  const SRange r = srange(L.len, L.per, gw);
  uint64_t j = lower64(L.starts, L.nmatch, r.lo, lane);  // next match to assign
  uint64_t line = 1 + L.prefix[gw];         // line of byte r.lo
  LineStats st;
  uint16_t* gm = gmask[wid];
  uint16_t* gp = gpre[wid];
  for (uint32_t i = 0; i < r.n && j < L.nmatch; ++i) {
    wave_sync();  // the previous tile's LDS reads precede these writes
    const uint64_t ts = r.lo + (uint64_t)i * kSTile;
    uint32_t c[4];
    const uint32_t base = tile_masks(L.g, r, i, lane, gm, gp, c);
    wave_sync();
    const uint64_t tend = ts + kSTile < r.hi ? ts + kSTile : r.hi;
    for (;;) {  // matches starting in this tile, 64 at a time
      const uint64_t idx = j + (uint64_t)lane;
      const uint64_t s = idx < L.nmatch ? L.starts[idx] : ~0ull;
      const bool in = s < tend;
      const uint64_t mb = __ballot(in);
      if (!mb) break;
      uint64_t ln = 0;
      if (in) {
        ln = line + rank_of(gm, gp, (uint32_t)(s - ts));
        if (L.lines) L.lines[idx] = ln;
      }
      st.add(ln, in, mb, lane);
      const uint32_t k = (uint32_t)__popcll(mb);
      j += k;
      if (k < 64) break;
    }
    line += base;
    if (j >= L.nmatch || L.starts[j] >= r.hi) break;  // no further match in this range
  }
  st.store(L.recs + gw, lane);
}

__global__ __launch_bounds__(kSWaves * 64) void nl_assign_sparse_kernel(LinesParams L)
{
  const int lane = threadIdx.x & 63;
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (gw >= L.nwaves) return;
  const SRange r = srange(L.len, L.per, gw);
  uint64_t j = lower64(L.starts, L.nmatch, r.lo, lane);
  uint64_t line = 1 + L.prefix[gw];
  LineStats st;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(L.g + r.lo), (short)0, __builtin_amdgcn_readfirstlane((int)r.rel16), 0x00020000);
  const uint32_t nquart = (r.rel + kLinesQuarter - 1) / kLinesQuarter;
  const uint16_t* qc = L.qcount + r.lo / kLinesQuarter;
  for (uint32_t qb = 0; qb < nquart && j < L.nmatch; qb += 64) {
    uint64_t s = L.starts[j];
    if (s >= r.hi) break;
    // line offsets of the next 64 quarters
    const uint32_t nq = nquart - qb < 64u ? nquart - qb : 64u;
    const uint32_t c = (uint32_t)lane < nq ? qc[qb + lane] : 0u;
    const uint32_t incl = lscan_add(c);
    const uint32_t excl = incl - c;
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane(incl, 63);
    const uint64_t bend0 = r.lo + (uint64_t)(qb + nq) * kLinesQuarter;
    const uint64_t bend = bend0 < r.hi ? bend0 : r.hi;
    while (s < bend) {  // each quarter holding a match start
      const uint32_t q = (uint32_t)((s - r.lo) / kLinesQuarter);
      const uint32_t qo = q * kLinesQuarter;
      const uint64_t qs = r.lo + qo;
      const uint64_t qe = qs + kLinesQuarter < r.hi ? qs + kLinesQuarter : r.hi;
      const uint64_t qline = line + (uint32_t)__builtin_amdgcn_readlane(excl, (int)(q - qb));
      const uint32_t go = qo + 16u * lane;
      const uint32_t m = nl16(sload16(rs, go)) & granule_valid(r.rel, go);
      const uint32_t cm = __popc(m);
      const uint32_t pre = lscan_add(cm) - cm;
      for (;;) {  // matches in this quarter, 64 at a time
        const uint64_t idx = j + (uint64_t)lane;
        const uint64_t sl = idx < L.nmatch ? L.starts[idx] : ~0ull;
        const bool in = sl < qe;
        const uint64_t mb = __ballot(in);
        if (!mb) break;  // the quarter held a multiple of 64 starts
        const uint32_t o = in ? (uint32_t)(sl - qs) : 0u;
        const int g = (int)(o >> 4);
        const uint32_t pg = (uint32_t)__shfl((int)pre, g, 64);  // all lanes take part
        const uint32_t mg = (uint32_t)__shfl((int)m, g, 64);
        const uint64_t ln = in ? qline + pg + __popc(mg & ((1u << (o & 15)) - 1u)) : 0ull;
        if (in && L.lines) L.lines[idx] = ln;
        st.add(ln, in, mb, lane);
        const uint32_t k = (uint32_t)__popcll(mb);
        j += k;
        if (k < 64) break;
      }
      s = j < L.nmatch ? L.starts[j] : ~0ull;
    }
    line += total;
  }
  st.store(L.recs + gw, lane);
}

hipError_t launch_nl_count(const LinesParams& L, bool sparse, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((L.nwaves + kSWaves - 1) / kSWaves);
  if (sparse)
    hipLaunchKernelGGL(nl_count_kernel<true>, dim3(grid), dim3(kSWaves * 64), 0, stream, L);
  else
    hipLaunchKernelGGL(nl_count_kernel<false>, dim3(grid), dim3(kSWaves * 64), 0, stream, L);
  return hipGetLastError();
}

hipError_t launch_nl_assign(const LinesParams& L, bool sparse, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((L.nwaves + kSWaves - 1) / kSWaves);
  if (sparse)
    hipLaunchKernelGGL(nl_assign_sparse_kernel, dim3(grid), dim3(kSWaves * 64), 0, stream, L);
  else
    hipLaunchKernelGGL(nl_assign_kernel, dim3(grid), dim3(kSWaves * 64), 0, stream, L);
  return hipGetLastError();
}

uint32_t lines_tile() { return kSTile; }

}  // namespace ugpu

// ---------------------------------------------------------------- C ABI
using namespace ugpu;

namespace {

// Per-call scratch of ugpu_lines beside the per-wave counts and prefixes:
// per-wave -c records with their pinned host copy, and quarter counts (sparse
// mode).
struct LinesWs : WaveWs {
  DevBuf<LineRec> d_rec;
  PinBuf<LineRec> h_rec;
  DevBuf<uint16_t> d_qc;

  hipError_t reserve(uint64_t nw, uint64_t quarters)
  {
    hipError_t e;
    if ((e = WaveWs::reserve(nw, 1)) != hipSuccess || (e = d_rec.reserve(nw, nw)) != hipSuccess ||
        (e = h_rec.reserve(nw, nw)) != hipSuccess)
      return e;
    return d_qc.reserve(quarters, quarters);
  }
};

}  // namespace

int ugpu_lines(const uint8_t* dbuf, uint64_t len, const uint64_t* d_start, uint64_t n, uint64_t* d_line,
               uint64_t* newlines, uint64_t* matching_lines, void* stream)
{
  if (!dbuf || (n && !d_start)) return fail(UGPU_INVAL, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dbuf) & 15u) return fail(UGPU_INVAL, "buffer must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint64_t per = 0, nw = 0;
  const int dev = line_wave_ranges(len, &per, &nw);
  if (dev < 0) return UGPU_DEVICE;
  // sparse assign pass when matches are rarer than one per two quarters
  // (UGPU_LINES_MODE=1/2 forces dense/sparse, for tests)
  const uint64_t quarters = (len + kSTile - 1) / kSTile * (kSTile / kLinesQuarter);
  bool sparse = n > 0 && n * 2 < quarters;
  if (const char* mo = getenv("UGPU_LINES_MODE")) {
    if (mo[0] == '1') sparse = false;
    if (mo[0] == '2') sparse = n > 0;
  }
  WsLease<LinesWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "lines workspace");
  hipError_t e = ws->reserve(nw, sparse ? quarters : 0);
  if (e != hipSuccess) return hip_fail(e, "lines buffers");
  LinesParams L = line_ranges_params(dbuf, len, per, nw);
  L.starts = d_start;
  L.nmatch = n;
  L.lines = d_line;
  L.counts = ws->d_out;
  L.prefix = ws->d_in;
  L.recs = ws->d_rec;
  L.qcount = sparse ? ws->d_qc : nullptr;
  uint64_t total = 0;
  if ((e = newline_prefix(*ws.ws, L, sparse, st, &total)) != hipSuccess) return hip_fail(e, "newline count");
  if (newlines) *newlines = total;
  if (n > 0 || matching_lines) {
    if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = launch_nl_assign(L, sparse, st)) != hipSuccess ||
        (e = hipMemcpyAsync(ws->h_rec, ws->d_rec, nw * sizeof(LineRec), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
      return hip_fail(e, "line assignment");
    // lines of consecutive matches in different waves may coincide
    uint64_t lines = 0, last = 0;
    bool any = false;
    for (uint64_t i = 0; i < nw; ++i) {
      const LineRec& r = ws->h_rec[i];
      if (!r.nmatch) continue;
      lines += r.trans;
      if (any && r.first_line == last) --lines;
      last = r.last_line;
      any = true;
    }
    if (matching_lines) *matching_lines = lines;
  }
  return UGPU_OK;
}
