// transcode.hip -- UTF-16/32, Latin-1, code-page and null-data input into the
// bytes the scans take.
//
// Replaces, for a fully buffered input, the conversion loops of
// Input::file_get (lib/input.cpp:748-1023); include/ugpu.h states the rules.
// Four of the five conversions are a per-unit length, a prefix sum and a
// scatter.  UTF-16 is not: a high surrogate (H, D800..DBFF) consumes the unit
// behind it whatever that is, so a unit is a character or a consumed second
// half by the parity of the run of H units before it.  With the bit "my first
// unit is consumed" coming in, a byte range hands the same bit on as one of
// constant 0, constant 1 (it ends in an H run that began inside it: the run's
// parity) or XOR with a parity (it is H units throughout).  Such a function is
// kept as its two values (bit c: the outgoing bit for the incoming bit c), which
// compose by a lookup: cf_compose().  Within a lane's 32 units the consumed
// units come from two carry-propagating adds over the H mask (seconds()),
// across lanes from a DPP scan of the lane functions, across tiles in
// registers, across wave ranges on the host (transcode_stitch, line_host.hpp).
// A range's output length depends on its incoming bit, so the summary pass
// follows both and reports two counts.
//
// Same wave-range layout as lines.hip (4 KiB tiles, tpw tiles per wave, a lane
// loads 64 consecutive bytes), over the bytes from `start`: the loads are
// dword aligned at start & ~3 and a funnel shift by start & 3 bytes lines the
// units up, so no unit straddles a lane.
//   tc_summary_kernel  per wave range: output bytes (UTF-16: for both incoming
//                      bits, and the range function);
//   (host)             transcode_stitch: output offset and incoming bit of
//                      each range, 64-bit;
//   tc_write_kernel    re-reads the range; per tile the lane totals are
//                      scanned, every lane writes its characters to the wave's
//                      LDS stage, and the stage goes out in whole 16-byte rows.
//                      The stage begins at the row of the range's output
//                      offset; the bytes of a last partial row stay at its
//                      front for the next tile.  The first and the last row
//                      of a range are shared with its neighbours: their bytes
//                      are stored one by one, by one lane each.
#include "device_common.hpp"
#include "line_host.hpp"
#include "line_tiles.hpp"

namespace ugpu {

namespace {

constexpr uint32_t kNonchar = 0x200000u;  // REFLEX_NONCHAR: utf8() gives F8 88 80 80 80
constexpr uint32_t kRaw = 0x80000000u;    // put(): the low byte as it is

constexpr bool is16(uint32_t enc) { return enc == UGPU_ENC_UTF16BE || enc == UGPU_ENC_UTF16LE; }
constexpr bool is32(uint32_t enc) { return enc == UGPU_ENC_UTF32BE || enc == UGPU_ENC_UTF32LE; }

// the largest output of a tile: 5 bytes per UTF-16 or UTF-32 unit, 2 per Latin-1 byte, 3 per code-page byte
constexpr uint32_t tile_out(uint32_t enc)
{
  return is16(enc) ? kSTile / 2 * 5 : is32(enc) ? kSTile / 4 * 5 : enc == UGPU_ENC_LATIN1 ? kSTile * 2
         : enc == UGPU_ENC_PAGE ? kSTile * 3 : kSTile;
}

// ---- range functions of UTF-16

// first f, then g
__device__ __forceinline__ uint32_t cf_compose(uint32_t f, uint32_t g)
{
  return ((g >> (f & 1u)) & 1u) | (((g >> ((f >> 1) & 1u)) & 1u) << 1);
}

template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t cf_dpp(uint32_t v)
{
  return (uint32_t)__builtin_amdgcn_update_dpp(2 /* the identity */, (int)v, CTRL, ROWS, 0xf, false);
}

// inclusive wave scan under cf_compose (the steps of lscan_add)
__device__ __forceinline__ uint32_t cf_scan(uint32_t v)
{
  v = cf_compose(cf_dpp<0x111, 0xf>(v), v);
  v = cf_compose(cf_dpp<0x112, 0xf>(v), v);
  v = cf_compose(cf_dpp<0x114, 0xf>(v), v);
  v = cf_compose(cf_dpp<0x118, 0xf>(v), v);
  v = cf_compose(cf_dpp<0x142, 0xa>(v), v);
  v = cf_compose(cf_dpp<0x143, 0xc>(v), v);
  return v;
}

// The consumed units of a lane: h has a bit per H unit (bits 0..31, only the
// lane's own units), c is the incoming bit.  Unit 0 is consumed iff c, and then
// takes part in no run; in a maximal run of H units from s, unit s + k is
// consumed for odd k, the unit behind the run included.  Adding the run starts
// at even (odd) positions to h flips exactly the runs that begin there and the
// bit behind each; the odd (even) positions of those are the consumed ones.
// Bit nu of the result, nu the lane's units, is the lane's outgoing bit.
__device__ __forceinline__ uint64_t seconds(uint32_t h32, uint32_t c)
{
  const uint64_t h = h32 & ~c;
  const uint64_t st = h & ~(h << 1);
  const uint64_t ce = (h + (st & 0x5555555555555555ull)) ^ h;
  const uint64_t co = (h + (st & 0xaaaaaaaaaaaaaaaaull)) ^ h;
  return (ce & 0xaaaaaaaaaaaaaaaaull) | (co & 0x5555555555555555ull) | c;
}

// ---- a lane's 64 bytes

struct Lane {
  uint32_t e[17];  // the lane's 16 dwords and the one behind them
  uint32_t own;    // its bytes inside the range (0..64)
  uint32_t avail;  // input bytes from its first byte on (capped at 128)
};

__device__ __forceinline__ Lane tc_load(const TcParams& P, const SRange& r, uint32_t i, int lane)
{
  const uint64_t tb = r.lo + (uint64_t)i * kSTile;
  const uint64_t left = P.readable - tb;  // (tb <= n <= readable - shift)
  const int nr = __builtin_amdgcn_readfirstlane((int)(left < (uint64_t)kSTile + 8 ? left : (uint64_t)kSTile + 8));
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(P.g + tb), (short)0, nr, 0x00020000);
  uint32_t d[18];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 v = sload16(rs, 64u * lane + 16u * k);
    d[4 * k] = v.x, d[4 * k + 1] = v.y, d[4 * k + 2] = v.z, d[4 * k + 3] = v.w;
  }
  typedef unsigned int v2u __attribute__((ext_vector_type(2)));
  const v2u t = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(64u * lane + 64u), 0, 0);
  d[16] = t.x, d[17] = t.y;
  Lane L;
  const uint32_t sh = 8u * P.shift;
#pragma unroll
  for (int k = 0; k < 17; ++k) L.e[k] = (uint32_t)(((((uint64_t)d[k + 1]) << 32) | d[k]) >> sh);
  const uint32_t pos = i * (uint32_t)kSTile + 64u * lane;  // from the range's first byte
  L.own = r.rel > pos ? (r.rel - pos < 64u ? r.rel - pos : 64u) : 0u;
  const uint64_t rest = P.n - r.lo;
  L.avail = rest > pos ? (uint32_t)(rest - pos < 128u ? rest - pos : 128u) : 0u;
  return L;
}

__device__ __forceinline__ uint32_t below32(uint32_t n) { return n >= 32u ? ~0u : (1u << n) - 1u; }

// ---- UTF-16

template <bool BE>
__device__ __forceinline__ uint32_t unit16(const Lane& L, int u)
{
  const uint32_t v = (L.e[u >> 1] >> (16 * (u & 1))) & 0xffffu;
  return BE ? ((v & 0xffu) << 8) | (v >> 8) : v;
}

struct U16 {
  uint32_t nu;    // the lane's units
  uint32_t vm;    // a bit per unit
  uint32_t h;     // H units
  uint32_t g1;    // units below 0x80
  uint32_t g2;    // units in 0x80..0x7FF
  uint32_t sur;   // surrogates
  uint32_t pair;  // H units with a low surrogate behind them
  uint32_t five;  // what gives NONCHAR when it is not consumed: the other H units, the low surrogates
};

template <bool BE>
__device__ __forceinline__ U16 classify16(const Lane& L)
{
  U16 c;
  uint32_t h = 0, g1 = 0, g2 = 0;
  uint64_t lo = 0;
#pragma unroll
  for (int u = 0; u < 33; ++u) {
    const uint32_t v = unit16<BE>(L, u);
    if ((v & 0xfc00u) == 0xdc00u) lo |= 1ull << u;
    if (u < 32) {
      if ((v & 0xfc00u) == 0xd800u) h |= 1u << u;
      if (v < 0x80u) g1 |= 1u << u;
      if (v >= 0x80u && v < 0x800u) g2 |= 1u << u;
    }
  }
  c.nu = L.own >> 1;
  c.vm = below32(c.nu);
  // the unit behind the lane's own ones exists when the input holds both its bytes
  const uint64_t in = (uint64_t)c.vm | (L.avail >= 2u * c.nu + 2u ? 1ull << c.nu : 0ull);
  lo &= in;
  c.h = h & c.vm;
  c.g1 = g1 & c.vm;
  c.g2 = g2 & c.vm;
  c.pair = c.h & (uint32_t)(lo >> 1);
  const uint32_t low = (uint32_t)lo & c.vm;
  c.sur = c.h | low;
  c.five = low | (c.h & ~c.pair);
  return c;
}

// the lane's function: its outgoing bit for both incoming bits
__device__ __forceinline__ uint32_t lane_fn(const U16& c)
{
  return (uint32_t)((seconds(c.h, 0) >> c.nu) & 1u) | ((uint32_t)((seconds(c.h, 1) >> c.nu) & 1u) << 1);
}

// output bytes of the units in m
__device__ __forceinline__ uint32_t total16(const U16& c, uint32_t m)
{
  const uint32_t m2 = m & ~c.g1, m3 = m2 & ~c.g2;
  return __popc(m) + __popc(m2) + __popc(m3) + __popc(m & c.sur) + __popc(m & c.five);
}

// ---- the other encodings: a unit's code point, kRaw | byte for a byte that passes as it is

template <uint32_t ENC>
__device__ __forceinline__ uint32_t units_of(const Lane& L)
{
  return is32(ENC) ? L.own >> 2 : L.own;
}

template <uint32_t ENC>
__device__ __forceinline__ uint32_t code_of(const Lane& L, int u, const uint16_t* pg)
{
  if (is32(ENC)) {
    const uint32_t v = L.e[u];
    const uint32_t c = ENC == UGPU_ENC_UTF32BE ? __builtin_bswap32(v) : v;
    return (int32_t)c < 0x80 ? kRaw | (c & 0xffu) : c;
  }
  const uint32_t b = (L.e[u >> 2] >> (8 * (u & 3))) & 0xffu;
  if (ENC == UGPU_ENC_LATIN1) return b;
  if (ENC == UGPU_ENC_PAGE) return pg[b];
  return kRaw | (b == 0u ? 10u : b == 10u ? 0u : b);  // null data
}

__device__ __forceinline__ uint32_t len_of(uint32_t cp)
{
  if ((cp & kRaw) || cp < 0x80u) return 1u;
  return cp < 0x800u ? 2u : cp < 0x10000u ? 3u : cp <= 0x10ffffu ? 4u : 5u;
}

template <uint32_t ENC>
__device__ __forceinline__ uint32_t lane_total(const Lane& L, const uint16_t* pg)
{
  constexpr int kUnits = is32(ENC) ? 16 : 64;
  const uint32_t nu = units_of<ENC>(L);
  if (ENC == UGPU_ENC_NULL_DATA) return nu;
  uint32_t t = 0;
#pragma unroll
  for (int u = 0; u < kUnits; ++u)
    if ((uint32_t)u < nu) t += len_of(code_of<ENC>(L, u, pg));
  return t;
}

// utf8(cp) to s[p...]; returns the position behind it
__device__ __forceinline__ uint32_t put(uint8_t* s, uint32_t p, uint32_t cp)
{
  if ((cp & kRaw) || cp < 0x80u) {
    s[p] = (uint8_t)cp;
    return p + 1u;
  }
  if (cp < 0x800u) {
    s[p] = (uint8_t)(0xc0u | (cp >> 6));
    s[p + 1] = (uint8_t)(0x80u | (cp & 0x3fu));
    return p + 2u;
  }
  if (cp < 0x10000u) {
    s[p] = (uint8_t)(0xe0u | (cp >> 12));
    s[p + 1] = (uint8_t)(0x80u | ((cp >> 6) & 0x3fu));
    s[p + 2] = (uint8_t)(0x80u | (cp & 0x3fu));
    return p + 3u;
  }
  if (cp <= 0x10ffffu) {
    s[p] = (uint8_t)(0xf0u | (cp >> 18));
    s[p + 1] = (uint8_t)(0x80u | ((cp >> 12) & 0x3fu));
    s[p + 2] = (uint8_t)(0x80u | ((cp >> 6) & 0x3fu));
    s[p + 3] = (uint8_t)(0x80u | (cp & 0x3fu));
    return p + 4u;
  }
  s[p] = 0xf8u, s[p + 1] = 0x88u, s[p + 2] = 0x80u, s[p + 3] = 0x80u, s[p + 4] = 0x80u;
  return p + 5u;
}

__device__ __forceinline__ void load_page(uint16_t* pg, const TcPage& page)
{
  pg[threadIdx.x] = page.v[threadIdx.x];  // (a block is 256 threads)
  __syncthreads();
}

}  // namespace

template <uint32_t ENC>
__global__ __launch_bounds__(kSWaves * 64) void tc_summary_kernel(TcParams P, TcPage page)
{
  static_assert(kSWaves * 64 == 256, "load_page: one entry per thread");
  __shared__ uint16_t pg[256];
  if (ENC == UGPU_ENC_PAGE) load_page(pg, page);
  const int lane = threadIdx.x & 63;
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (gw >= P.nwaves) return;
  const SRange r = srange(P.n, P.per, gw);
  uint32_t t0 = 0, t1 = 0;  // output bytes, per lane (a range gives less than 2^32)
  uint32_t c0 = 0, c1 = 1;  // UTF-16: the bit at the tile's first unit, for the range's incoming bit 0 and 1
  for (uint32_t i = 0; i < r.n; ++i) {
    const Lane L = tc_load(P, r, i, lane);
    if constexpr (is16(ENC)) {
      const U16 c = classify16<ENC == UGPU_ENC_UTF16BE>(L);
      const uint32_t incl = cf_scan(lane_fn(c));
      const uint32_t up = __shfl_up(incl, 1, 64);
      const uint32_t before = lane ? up : 2u;  // the function of the tile's units before the lane's
      t0 += total16(c, c.vm & ~(uint32_t)seconds(c.h, (before >> c0) & 1u));
      t1 += total16(c, c.vm & ~(uint32_t)seconds(c.h, (before >> c1) & 1u));
      const uint32_t F = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      c0 = (F >> c0) & 1u, c1 = (F >> c1) & 1u;
    } else {
      t0 += lane_total<ENC>(L, pg);
    }
  }
  const uint64_t s0 = wave_sum((uint64_t)t0);
  const uint64_t s1 = wave_sum((uint64_t)t1);
  if (lane == 0) {
    P.cnt0[gw] = s0;
    if constexpr (is16(ENC)) {
      P.cnt1[gw] = s1;
      P.fn[gw] = c0 | (c1 << 1);
    }
  }
}

template <uint32_t ENC>
__global__ __launch_bounds__(kSWaves * 64) void tc_write_kernel(TcParams P, TcPage page)
{
  constexpr uint32_t kStage = 16 + tile_out(ENC);  // up to 15 bytes of the row before, and a tile's output
  __shared__ uint4 stage4[kSWaves][kStage / 16];
  __shared__ uint16_t pg[256];
  if (ENC == UGPU_ENC_PAGE) load_page(pg, page);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + wid;
  if (gw >= P.nwaves) return;
  const SRange r = srange(P.n, P.per, gw);
  uint8_t* const stage = reinterpret_cast<uint8_t*>(stage4[wid]);
  const uint64_t ob = P.obase[gw];
  uint64_t row = ob & ~15ull;        // output offset of stage[0]
  uint32_t a = (uint32_t)(ob & 15u);  // bytes at the front of the stage that the coming tile does not write
  uint32_t skip = a;                 // those of them that belong to the range before (first row only)
  uint32_t cin = is16(ENC) ? (uint32_t)P.cin[gw] : 0u;
  for (uint32_t i = 0; i < r.n; ++i) {
    const Lane L = tc_load(P, r, i, lane);
    uint32_t tot, emit = 0;  // emit: the lane's units that are not consumed
    U16 c{};
    if constexpr (is16(ENC)) {
      c = classify16<ENC == UGPU_ENC_UTF16BE>(L);
      const uint32_t incl = cf_scan(lane_fn(c));
      const uint32_t up = __shfl_up(incl, 1, 64);
      const uint32_t before = lane ? up : 2u;
      emit = c.vm & ~(uint32_t)seconds(c.h, (before >> cin) & 1u);
      tot = total16(c, emit);
      cin = ((uint32_t)__builtin_amdgcn_readlane((int)incl, 63) >> cin) & 1u;
    } else {
      tot = lane_total<ENC>(L, pg);
    }
    const uint32_t incl = lscan_add(tot);
    const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    wave_sync();  // the previous tile's stage reads and its move to the front precede these writes
    uint32_t p = a + incl - tot;
    if constexpr (is16(ENC)) {
#pragma unroll
      for (int u = 0; u < 32; ++u)
        if ((emit >> u) & 1u) {
          const uint32_t v = unit16<ENC == UGPU_ENC_UTF16BE>(L, u);
          uint32_t cp = v;
          if ((c.sur >> u) & 1u)
            cp = (c.pair >> u) & 1u
                     ? 0x10000u + ((v - 0xd800u) << 10) + (unit16<ENC == UGPU_ENC_UTF16BE>(L, u + 1) - 0xdc00u)
                     : kNonchar;
          p = put(stage, p, cp);
        }
    } else {
      constexpr int kUnits = is32(ENC) ? 16 : 64;
      const uint32_t nu = units_of<ENC>(L);
#pragma unroll
      for (int u = 0; u < kUnits; ++u)
        if ((uint32_t)u < nu) p = put(stage, p, code_of<ENC>(L, u, pg));
    }
    wave_sync();
    const uint32_t total = a + T, full = total >> 4;
    if (full) {
      for (uint32_t k = lane; k < full; k += 64) {
        if (k == 0 && skip) {  // the range's first row: the bytes before `skip` are the previous range's
          for (uint32_t b = skip; b < 16u; ++b) P.dst[row + b] = stage[b];
        } else {
          *reinterpret_cast<uint4*>(P.dst + row + 16ull * k) = stage4[wid][k];
        }
      }
      const uint32_t rem = total & 15u;
      const uint8_t t = (uint32_t)lane < rem ? stage[16u * full + lane] : (uint8_t)0;
      wave_sync();  // the rows are read
      if ((uint32_t)lane < rem) stage[lane] = t;
      row += 16ull * full;
      a = rem;
      skip = 0;
    } else {
      a = total;
    }
  }
  wave_sync();
  // the range's last row, shared with the range behind
  if ((uint32_t)lane >= skip && (uint32_t)lane < a) P.dst[row + lane] = stage[lane];
}

namespace {

template <uint32_t ENC>
void summary_of(const TcParams& P, const TcPage& page, uint32_t grid, hipStream_t st)
{
  hipLaunchKernelGGL(tc_summary_kernel<ENC>, dim3(grid), dim3(kSWaves * 64), 0, st, P, page);
}

template <uint32_t ENC>
void write_of(const TcParams& P, const TcPage& page, uint32_t grid, hipStream_t st)
{
  hipLaunchKernelGGL(tc_write_kernel<ENC>, dim3(grid), dim3(kSWaves * 64), 0, st, P, page);
}

}  // namespace

#define TC_DISPATCH(fn)                                                       \
  switch (P.enc) {                                                            \
    case UGPU_ENC_UTF16BE: fn<UGPU_ENC_UTF16BE>(P, page, grid, stream); break; \
    case UGPU_ENC_UTF16LE: fn<UGPU_ENC_UTF16LE>(P, page, grid, stream); break; \
    case UGPU_ENC_UTF32BE: fn<UGPU_ENC_UTF32BE>(P, page, grid, stream); break; \
    case UGPU_ENC_UTF32LE: fn<UGPU_ENC_UTF32LE>(P, page, grid, stream); break; \
    case UGPU_ENC_LATIN1: fn<UGPU_ENC_LATIN1>(P, page, grid, stream); break;   \
    case UGPU_ENC_PAGE: fn<UGPU_ENC_PAGE>(P, page, grid, stream); break;       \
    case UGPU_ENC_NULL_DATA: fn<UGPU_ENC_NULL_DATA>(P, page, grid, stream); break; \
    default: return hipErrorInvalidValue;                                     \
  }

hipError_t launch_tc_summary(const TcParams& P, const TcPage& page, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((P.nwaves + kSWaves - 1) / kSWaves);
  TC_DISPATCH(summary_of)
  return hipGetLastError();
}

hipError_t launch_tc_write(const TcParams& P, const TcPage& page, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((P.nwaves + kSWaves - 1) / kSWaves);
  TC_DISPATCH(write_of)
  return hipGetLastError();
}

#undef TC_DISPATCH

}  // namespace ugpu

// ---------------------------------------------------------------- C ABI
using namespace ugpu;

int ugpu_transcode(const uint8_t* dbuf, uint64_t len, uint64_t start, uint32_t enc, const uint16_t* page,
                   uint8_t* d_dst, uint64_t capacity, uint64_t* out_len, void* stream)
{
  if (enc == UGPU_ENC_PLAIN || enc == UGPU_ENC_UTF8) return fail(UGPU_INVAL, "nothing to convert for this encoding");
  if (enc > UGPU_ENC_NULL_DATA) return fail(UGPU_INVAL, "unknown encoding");
  if (enc == UGPU_ENC_PAGE && !page) return fail(UGPU_INVAL, "a code page needs its table");
  if (enc != UGPU_ENC_PAGE && page) return fail(UGPU_INVAL, "a page table goes with UGPU_ENC_PAGE only");
  if (start > len) return fail(UGPU_INVAL, "start lies behind the input");
  if (!dbuf || !out_len) return fail(UGPU_INVAL, "NULL argument");
  if ((reinterpret_cast<uintptr_t>(dbuf) | reinterpret_cast<uintptr_t>(d_dst)) & 15u)
    return fail(UGPU_INVAL, "buffers must be 16-byte aligned");
  *out_len = 0;
  if (len == start) return UGPU_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  TcParams P{};
  P.g = dbuf + (start & ~3ull);
  P.shift = (uint32_t)(start & 3u);
  P.enc = enc;
  P.n = len - start;
  P.readable = ((len + 15u) & ~15ull) - (start & ~3ull);
  const int dev = line_wave_ranges(P.n, &P.per, &P.nwaves);
  if (dev < 0) return UGPU_DEVICE;
  WsLease<WaveWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "transcode workspace");
  const uint64_t nw = P.nwaves;
  hipError_t e = ws->reserve(nw, 3);
  if (e != hipSuccess) return hip_fail(e, "transcode buffers");
  TcPage pg{};
  if (page)
    for (int i = 0; i < 256; ++i) pg.v[i] = page[i];
  P.cnt0 = ws->d_out;
  P.cnt1 = ws->d_out + nw;
  P.fn = ws->d_out + 2 * nw;
  P.obase = ws->d_in;
  P.cin = ws->d_in + nw;
  P.dst = d_dst;
  const bool carry = is16(enc);
  const uint64_t back = carry ? 3 : 1;
  if ((e = launch_tc_summary(P, pg, st)) != hipSuccess ||
      (e = hipMemcpyAsync(ws->h_out, ws->d_out, nw * back * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "transcode summary");
  *out_len = transcode_stitch(ws->h_out, ws->h_in, nw, carry);
  if (!d_dst) return UGPU_OK;
  if (*out_len > capacity) return fail(UGPU_CAPACITY, "transcode destination too small");
  if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * 2 * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = launch_tc_write(P, pg, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "transcode write");
  return UGPU_OK;
}
