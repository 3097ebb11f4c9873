// ngram.hpp -- the n-gram candidate filter of kernel 7 (ngram_kernel.hip),
// one text for host and device.
//
// For a table whose shortest match has at least 2 bytes, n = min(shortest
// match, 4) and G = the n-byte strings that begin a match (the DFA's paths of
// depth n from the start state; none passes an accepting state).  A position p
// can start a match only if bytes p .. p+n-1 are in G.  G is kept as a hashed
// bitmap of 2^k bits: bit ngram_hash(window) is set for every member, so a
// member always tests positive (superset) and a non-member tests positive at
// about the bitmap's fill ratio.
//
// The window of position p is its n bytes packed little-endian (byte p in bits
// 0-7), bytes past n zero.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UGPU_HD __host__ __device__ __forceinline__
#else
#define UGPU_HD inline
#endif

namespace ugpu {

constexpr uint32_t kNgMaxN = 4;
constexpr uint32_t kNgMinLog2 = 12, kNgMaxLog2 = 18;  // bitmap bits: 512 B .. 32 KiB of LDS
constexpr uint32_t kNgMaxGrams = 1u << 16;            // the enumeration gives up above this (then a smaller n)

// the bytes of a window that count for n-grams of n bytes
UGPU_HD uint32_t ngram_mask(uint32_t n) { return n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u; }

// Fibonacci hashing: the top k bits of the product depend on every window bit,
// so windows that differ in one byte (text) spread over the whole bitmap and
// the lanes' dword gathers over the LDS banks
UGPU_HD uint32_t ngram_hash(uint32_t window, uint32_t log2_bits) { return (window * 0x9E3779B1u) >> (32u - log2_bits); }

// window: already masked with ngram_mask(n)
UGPU_HD bool ngram_test(const uint32_t* bitmap, uint32_t window, uint32_t log2_bits)
{
  const uint32_t h = ngram_hash(window, log2_bits);
  return (bitmap[h >> 5] >> (h & 31u)) & 1u;
}

}  // namespace ugpu
