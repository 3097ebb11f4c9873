// line_tiles.hpp -- device helpers of the line kernels (lines.hip, linesel.hip,
// linebool.hip): the 4 KiB tile loads, the 16-byte granule newline masks with
// their prefix, rank_of / mark / select_nl on them, the wave scans and the
// 64-ary search of a sorted match list.  Everything is per wave.
#pragma once
#include <cstdint>

#include "device_common.hpp"

namespace ugpu {

namespace {

constexpr int kSTile = 4096;
constexpr int kSWaves = 4;
constexpr int kTbWords = 132;  // line bits of a tile: ranks 0..4096, one spare word, a multiple of 4

__device__ __forceinline__ uint4 sload16(__amdgpu_buffer_rsrc_t rs, uint32_t off)
{
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 2 /* nt */);
  return uint4{v.x, v.y, v.z, v.w};
}

// bit 7 of each byte set iff the byte is '\n' (exact: no carries between bytes)
__device__ __forceinline__ uint32_t nl_bits(uint32_t x)
{
  const uint32_t t = x ^ 0x0a0a0a0au;
  const uint32_t nz = ((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t;
  return ~nz & 0x80808080u;
}

__device__ __forceinline__ uint32_t nl4(uint32_t x) { return ((nl_bits(x) >> 7) * 0x01020408u) >> 24; }

__device__ __forceinline__ uint32_t nl16(const uint4& v)
{
  return nl4(v.x) | (nl4(v.y) << 4) | (nl4(v.z) << 8) | (nl4(v.w) << 12);
}

// Tile i of the range starting at wbase (rel = readable bytes from wbase).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ltile(const uint8_t* wbase, uint32_t i, uint32_t rel)
{
  const uint32_t off = i * (uint32_t)kSTile;
  const uint32_t n = rel > off ? rel - off : 0u;
  const int nr = __builtin_amdgcn_readfirstlane((int)(n < (uint32_t)kSTile ? n : (uint32_t)kSTile));
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(wbase + off), (short)0, nr, 0x00020000);
}

// inclusive wave scans (DPP; 0 is the identity of both)
__device__ __forceinline__ uint32_t lscan_add(uint32_t v)
{
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint32_t lscan_max(uint32_t v)
{
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));
  return v;
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

struct SRange {
  uint64_t lo, hi;  // byte range [lo, hi) of this wave
  uint32_t n;       // tiles
  uint32_t rel;     // bytes of the range (hi - lo)
  uint32_t rel16;   // rel rounded up to 16: the loads' bound (a buffer load
                    // past num_records zeroes the whole dword, so a ragged end
                    // is loaded whole, inside the aligned 16-byte granule, and
                    // masked with granule_valid)
};

// 16-bit mask of the bytes of granule [off, off+16) that lie below rel
__device__ __forceinline__ uint32_t granule_valid(uint32_t rel, uint32_t off)
{
  const uint32_t rem = rel > off ? rel - off : 0u;
  return rem >= 16u ? 0xffffu : (1u << rem) - 1u;
}

__device__ __forceinline__ SRange srange(uint64_t len, uint64_t per, uint64_t gw)
{
  SRange r;
  r.lo = gw * per;
  if (r.lo > len) r.lo = len;
  r.hi = r.lo + per < len ? r.lo + per : len;
  r.n = (uint32_t)((r.hi - r.lo + kSTile - 1) / kSTile);
  r.rel = (uint32_t)(r.hi - r.lo);
  r.rel16 = (r.rel + 15u) & ~15u;
  return r;
}

// First index of the sorted list a[0, n) with a[idx] >= key: 64-ary search.
__device__ __forceinline__ uint64_t lower64(const uint64_t* a, uint64_t n, uint64_t key, int lane)
{
  uint64_t lo = 0, hi = n;  // answer in [lo, hi]
  while (hi - lo > 64) {
    const uint64_t step = (hi - lo + 63) / 64;
    const uint64_t idx = lo + step * (uint64_t)lane;
    const bool below = idx < hi && a[idx] < key;
    const int cntb = __popcll(__ballot(below));  // pivots below key (a prefix of the lanes)
    const uint64_t nlo = cntb ? lo + step * (uint64_t)(cntb - 1) + 1 : lo;
    const uint64_t nhi = lo + step * (uint64_t)cntb;
    lo = nlo;
    hi = nhi < hi ? nhi : hi;
  }
  const uint64_t idx = lo + (uint64_t)lane;
  const bool below = idx < hi && a[idx] < key;
  return lo + __popcll(__ballot(below));
}

// Newline masks of tile i into gm (granule g = 64 k + lane), their exclusive
// prefix into gp, per-lane counts in c[]; returns the tile's newline count.
__device__ __forceinline__ uint32_t tile_masks(const uint8_t* g, const SRange& r, uint32_t i, int lane, uint16_t* gm,
                                               uint16_t* gp, uint32_t (&c)[4])
{
  const __amdgpu_buffer_rsrc_t rs = ltile(g + r.lo, i, r.rel16);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t o = 16u * lane + 1024u * k;
    const uint32_t m = nl16(sload16(rs, o)) & granule_valid(r.rel, i * (uint32_t)kSTile + o);
    gm[64 * k + lane] = (uint16_t)m;
    c[k] = __popc(m);
  }
  uint32_t base = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t incl = lscan_add(c[k]);
    gp[64 * k + lane] = (uint16_t)(base + incl - c[k]);
    base += (uint32_t)__builtin_amdgcn_readlane(incl, 63);
  }
  return base;
}

__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// newlines of the tile before its byte x (< 4096): the rank of x's line in the tile
__device__ __forceinline__ uint32_t rank_of(const uint16_t* gm, const uint16_t* gp, uint32_t x)
{
  const uint32_t g = x >> 4;
  return (uint32_t)gp[g] + __popc((uint32_t)gm[g] & ((1u << (x & 15u)) - 1u));
}

// set the line bits r0..r1 (r0 <= r1 <= 4096)
__device__ __forceinline__ void mark(uint32_t* tb, uint32_t r0, uint32_t r1)
{
  const uint32_t w0 = r0 >> 5, w1 = r1 >> 5;
  const uint32_t first = ~((1u << (r0 & 31u)) - 1u), last = (2u << (r1 & 31u)) - 1u;
  if (w0 == w1) {
    atomicOr(&tb[w0], first & last);
  } else {
    atomicOr(&tb[w0], first);
    for (uint32_t w = w0 + 1; w < w1; ++w) atomicOr(&tb[w], ~0u);
    atomicOr(&tb[w1], last);
  }
}

// tile offset of the rk-th (1-based, <= the tile's count) newline of the tile
__device__ __forceinline__ uint32_t select_nl(const uint16_t* gm, const uint16_t* gp, uint32_t rk)
{
  uint32_t g = 0;  // the last granule with fewer than rk newlines before it holds the rk-th
#pragma unroll
  for (uint32_t step = 128; step; step >>= 1)
    if ((uint32_t)gp[g + step] < rk) g += step;
  uint32_t m = gm[g];
  for (uint32_t t = rk - (uint32_t)gp[g]; t > 1; --t) m &= m - 1u;
  return 16u * g + (uint32_t)__builtin_ctz(m);
}

}  // namespace

}  // namespace ugpu
