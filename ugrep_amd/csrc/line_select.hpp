// line_select.hpp -- the steps of the line selection walk that sel_kernel
// (linesel.hip, one match list) and bool_kernel (linebool.hip, K lists) share,
// and those of their summary kernels.  Per wave, over the tile state of
// line_tiles.hpp: gm / gp (granule newline masks and their prefix), tb (one bit
// per line of the tile), the tile's bytes [ts, tend).
//
// Only steps that leave the kernels' generated code as it is are here: scalar
// arguments and results, no arrays handed over by reference.  The write pass's
// two scans with its record loop, and the advance of the open line, stay in the
// two kernel bodies: as shared functions over field[] / lp[] they changed the
// schedule and the SGPR spills of bool_kernel<*,16> (146 VGPRs, ~145 spilled
// SGPRs) and cost it 0.3-1 %.
#pragma once
#include "line_tiles.hpp"

namespace ugpu {

namespace {

// 1 + position of the range's last newline (0: none): tiles walked from the end
__device__ __forceinline__ uint64_t last_newline(const uint8_t* g, const SRange& r, int lane)
{
  for (uint32_t i = r.n; i-- > 0;) {
    const __amdgpu_buffer_rsrc_t rs = ltile(g + r.lo, i, r.rel16);
    uint32_t best = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t o = 16u * lane + 1024u * k;
      const uint32_t m = nl16(sload16(rs, o)) & granule_valid(r.rel, i * (uint32_t)kSTile + o);
      if (m) best = umax(best, o + 32u - (uint32_t)__builtin_clz(m));
    }
    best = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max(best));
    if (best) return r.lo + (uint64_t)i * kSTile + best;
  }
  return 0;
}

// Exclusive end of the bytes match idx (start s < len) touches: a zero-length
// match touches byte s.
__device__ __forceinline__ uint64_t match_end(const uint32_t* lens, uint64_t len, uint64_t idx, uint64_t s)
{
  const uint64_t l = lens ? (uint64_t)lens[idx] : 0ull;
  const uint64_t e = l ? s + l : s + 1;
  return e < len ? e : len;
}

// largest exclusive end of the matches of one list that start in the range
__device__ __forceinline__ uint64_t range_cover(const uint64_t* starts, const uint32_t* lens, uint64_t n, uint64_t len,
                                                const SRange& r, int lane)
{
  const uint64_t j0 = lower64(starts, n, r.lo, lane), j1 = lower64(starts, n, r.hi, lane);
  uint64_t cv = 0;
  for (uint64_t idx = j0 + (uint64_t)lane; idx < j1; idx += 64) {
    const uint64_t e = match_end(lens, len, idx, starts[idx]);
    cv = e > cv ? e : cv;
  }
  return wave_max(cv);
}

// the open line and the lines after it that earlier matches (reaching to cover) touch
__device__ __forceinline__ void mark_cover(uint32_t* tb, const uint16_t* gm, const uint16_t* gp, uint64_t cover,
                                           uint64_t bol, uint64_t ts, uint64_t tend, int lane)
{
  if (cover > bol && lane == 0) {
    uint32_t hr = 0;
    if (cover > ts) hr = rank_of(gm, gp, (uint32_t)((cover < tend ? cover : tend) - 1 - ts));
    mark(tb, 0, hr);
  }
}

// Marks the lines touched by the matches of one list that start in the tile,
// from match j on, 64 at a time; returns the next match index (j itself: none
// started here) and leaves in cl this lane's share of their largest exclusive
// end (the tile's cover is its wave_max).
__device__ __forceinline__ uint64_t place_matches(uint32_t* tb, const uint16_t* gm, const uint16_t* gp,
                                                  const uint64_t* starts, const uint32_t* lens, uint64_t n,
                                                  uint64_t len, uint64_t j, uint64_t ts, uint64_t tend, int lane,
                                                  uint64_t& cl)
{
  cl = 0;
  for (;;) {
    const uint64_t idx = j + (uint64_t)lane;
    const uint64_t s = idx < n ? starts[idx] : ~0ull;
    const bool in = s < tend;
    const uint64_t mb = __ballot(in);
    if (!mb) break;
    uint32_t r0 = 0, r1 = 0;
    if (in) {
      const uint64_t e = match_end(lens, len, idx, s);
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
  return j;
}

// The lines ending in a tile: granule g's are ranks r0 = gp[g] .. r0 + c - 1.
// Their bits of the finished bitmap, xored with inv.
__device__ __forceinline__ uint32_t granule_field(const uint32_t* tb, uint32_t r0, uint32_t c, uint32_t inv)
{
  const uint64_t two = (uint64_t)tb[r0 >> 5] | ((uint64_t)tb[(r0 >> 5) + 1] << 32);
  return ((uint32_t)(two >> (r0 & 31u)) ^ inv) & ((1u << c) - 1u);
}

// 1 + tile offset of granule g's last newline (0: it has none)
__device__ __forceinline__ uint32_t last_in_granule(const uint16_t* gm, uint32_t g)
{
  const uint32_t m = gm[g];
  return m ? 16u * g + 32u - (uint32_t)__builtin_clz(m) : 0u;
}

// The unterminated last line [bol, len), when it is selected: its record
// (write pass) or one more line for the wave's count.
template <bool WRITE>
__device__ __forceinline__ void tail_line(uint64_t bol, uint64_t len, uint64_t line, uint64_t out, int lane,
                                          uint64_t* begin, uint64_t* end, uint64_t* lineno, uint64_t& total)
{
  if (WRITE) {
    if (lane == 0) {
      begin[out] = bol;
      end[out] = len;
      lineno[out] = line;
    }
  } else {
    ++total;
  }
}

}  // namespace

}  // namespace ugpu
