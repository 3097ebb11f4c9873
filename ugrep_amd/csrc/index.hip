// index.hip -- the file index of ugrep-indexer on the device (include/ugpu.h,
// ugpu_index_tables / ugpu_index_batch).
//
// Per input (a segment of one packed buffer) the reference keeps a table of
// 65536 bytes, all ones, and clears bit k of table[h(i, k)] for every position
// i and k in 0..7 with i + k inside the input, h(i, 0) = byte[i] and
// h(i, k) = 61 h(i, k-1) + byte[i+k] mod 2^16.  Then it halves the table (AND
// of the halves) while the zero bits of the half stay under max_noise percent.
//
// A workgroup owns one table in LDS and clears bits with ds_and on dwords.  AND
// is idempotent and order-free, so the result does not depend on the schedule.
// Folding to `size` bytes is the same as indexing the table with h mod size, so
// a segment whose final table is bounded by `size` (at most 8n bits are
// cleared, which folds every half above 100 n / max_noise for certain) hashes
// into a table of that size from the start.  A segment of up to kIdxChunk bytes
// is hashed, folded and counted by one workgroup; a larger one is cut into
// chunks whose tables are ANDed into one table in global memory (dwords still
// all ones are skipped), and a fold launch follows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "hip_host.hpp"

namespace ugpu {

namespace {

constexpr uint32_t kIdxThreads = 1024;          // 16 waves: two workgroups per CU by LDS
constexpr uint32_t kIdxWaves = kIdxThreads / 64;
constexpr uint64_t kIdxChunk = 256ull << 10;    // bytes one workgroup hashes
constexpr uint32_t kIdxTable = 65536;           // the unfolded table
constexpr uint32_t kIdxMin = 128;               // the smallest table
constexpr uint32_t kIdxWindow = 65536;          // the bytes the binary flag looks at
constexpr uint32_t kIdxFlagThreads = 256;
constexpr uint32_t kNoGlob = 0xffffffffu;

constexpr uint32_t kMaxNoise[10] = {80, 73, 65, 57, 49, 42, 34, 26, 18, 10};  // noise_percentage(), by accuracy

struct IdxSeg {
  uint64_t beg, end;  // bytes of the buffer
  uint64_t slot;      // its table's place in the slots, bytes
  uint32_t logb;      // log2 of the table it hashes into (the sizing bound)
  uint32_t glob;      // a segment of several chunks: its table in global memory; kNoGlob otherwise
};
struct IdxWork {
  uint32_t seg, chunk;
};
struct IdxOut {
  uint32_t header;  // log2 of the final table (0: none) | binary << 7
  uint32_t zeros;   // zero bits of the final table
};
struct IdxParams {
  const uint8_t* g;
  const IdxSeg* seg;
  const IdxWork* work;
  const uint32_t* gseg;  // fold launch: the segment of each global table
  uint32_t* flag;        // per segment: binary
  IdxOut* out;
  uint8_t* slots;
  uint32_t* glob;        // kIdxTable / 4 dwords per global table
  const uint64_t* off;   // emit launch: each segment's offset in dst
  uint8_t* dst;
  uint32_t max_noise;
  uint32_t ignore_binary;
};

// ---- the binary flag (ugrep-indexer.cpp:782-803 and :892-902) over the first
// window.  The sequential check never fails iff every byte passes a local one:
// a NUL and a byte in C0, C1, F5..FF fail; a lead C2..F4 needs its 1-3
// continuation bytes inside the window; a continuation byte needs a lead 1-3
// bytes before it that reaches it over continuation bytes only.
__device__ inline uint32_t lead_need(uint32_t c) { return 1u + (c >= 0xE0u) + (c >= 0xF0u); }

__global__ __launch_bounds__(kIdxFlagThreads) void idx_flag_kernel(IdxParams P)
{
  const IdxSeg S = P.seg[blockIdx.x];
  const uint8_t* w = P.g + S.beg;
  const uint64_t n = S.end - S.beg;
  __shared__ uint32_t s_end, s_bin;
  if (threadIdx.x == 0) {
    uint32_t end = (uint32_t)(n < kIdxWindow ? n : kIdxWindow), bin = 0;
    if (end && (w[end - 1] & 0x80u)) {
      // the window's last sequence is cut off, complete or not
      uint32_t k = end < 4 ? end : 4;
      while (k > 0 && (w[--end] & 0xC0u) == 0x80u) --k;
      bin = (w[end] & 0xC0u) != 0xC0u;
    }
    s_end = end;
    s_bin = bin;
  }
  __syncthreads();
  const uint32_t end = s_end;
  uint32_t bad = 0;
  for (uint32_t p = threadIdx.x; p < end; p += kIdxFlagThreads) {
    const uint32_t b = w[p];
    if (b - 1u < 0x7Fu) continue;
    if (b < 0x80u || b > 0xF4u || (b & 0xFEu) == 0xC0u) {
      bad = 1;
    } else if (b >= 0xC2u) {
      const uint32_t need = lead_need(b);
      for (uint32_t q = 1; q <= need; ++q)
        if (p + q >= end || (w[p + q] & 0xC0u) != 0x80u) bad = 1;
    } else {
      bool ok = false;
      for (uint32_t j = 1; j <= 3 && j <= p; ++j) {
        const uint32_t c = w[p - j];
        if ((c & 0xC0u) == 0x80u) continue;
        ok = c >= 0xC2u && c <= 0xF4u && lead_need(c) >= j;
        break;
      }
      if (!ok) bad = 1;
    }
  }
  if (bad) atomicOr(&s_bin, 1u);
  __syncthreads();
  if (threadIdx.x == 0) P.flag[blockIdx.x] = s_bin;
}

// ---- hash, fold, count
__device__ inline uint32_t block_sum(uint32_t v, uint32_t* s_red)
{
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63u) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  for (uint32_t i = 0; i < kIdxWaves; ++i) t += s_red[i];
  __syncthreads();
  return t;
}

// The noise rule on tab[0, 2^logb bytes), in order from the largest table down
// (ugrep-indexer.cpp:997-1027), then the final table to the segment's slot.
// The reference compares 100 * (z / (8 half)) with max_noise in float; z is
// below 2^24 and 8 half a power of two, so 100 z >= max_noise * 8 half decides
// the same.
__device__ void fold_store(uint32_t* tab, uint32_t* s_red, uint32_t logb, uint32_t seg, const IdxSeg& S,
                           const IdxParams& P)
{
  uint32_t size = 1u << logb;
  uint32_t local = 0;
  for (uint32_t i = threadIdx.x; i < size / 4; i += kIdxThreads) local += __popc(~tab[i]);
  uint32_t z = block_sum(local, s_red);
  while (size > kIdxMin) {
    const uint32_t half = size / 2, hd = half / 4;
    local = 0;
    for (uint32_t i = threadIdx.x; i < hd; i += kIdxThreads) local += __popc(~(tab[i] & tab[i + hd]));
    const uint32_t zh = block_sum(local, s_red);
    if (100ull * zh >= (uint64_t)P.max_noise * 8u * half) break;
    for (uint32_t i = threadIdx.x; i < hd; i += kIdxThreads) tab[i] &= tab[i + hd];
    __syncthreads();
    size = half;
    z = zh;
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(P.slots + S.slot);
  for (uint32_t i = threadIdx.x; i < size / 4; i += kIdxThreads) dst[i] = tab[i];
  if (threadIdx.x == 0) {
    IdxOut o;
    o.header = (31u - (uint32_t)__clz((int)size)) | (P.flag[seg] << 7);
    o.zeros = z;
    P.out[seg] = o;
  }
}

template <bool FULL>
__device__ inline void hash_four(uint32_t* tab, uint32_t mask, uint32_t d0, uint32_t d1, uint32_t d2, uint64_t off,
                                 uint64_t lo, uint64_t hi, uint64_t end)
{
  const uint64_t w01 = (uint64_t)d0 | ((uint64_t)d1 << 32);
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint64_t pos = off + j;
    if (!FULL && (pos < lo || pos >= hi)) continue;
    const uint32_t lim = FULL ? 8u : (uint32_t)(end - pos < 8 ? end - pos : 8);
    // bytes j .. j+7 of the 12 in d0 d1 d2
    const uint64_t a = w01 >> (8 * j);
    const uint32_t blo = (uint32_t)a, bhi = (uint32_t)(a >> 32) | (j ? d2 << (32 - 8 * j) : 0u);
    uint32_t h = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      const uint32_t b = ((k < 4 ? blo : bhi) >> (8 * (k & 3u))) & 0xFFu;
      h = (61u * h + b) & 0xFFFFu;
      if (FULL || k < lim) {
        const uint32_t idx = h & mask;
        atomicAnd(&tab[idx >> 2], ~(1u << ((idx & 3u) * 8u + k)));
      }
    }
  }
}

__global__ __launch_bounds__(kIdxThreads) void idx_hash_kernel(IdxParams P)
{
  __shared__ uint32_t tab[kIdxTable / 4];
  __shared__ uint32_t s_red[kIdxWaves];
  const IdxWork W = P.work[blockIdx.x];
  const IdxSeg S = P.seg[W.seg];
  const bool multi = S.glob != kNoGlob;
  if (P.ignore_binary && P.flag[W.seg]) {  // -I: no table (a segment of several chunks: the fold launch says so)
    if (!multi && threadIdx.x == 0) {
      IdxOut o;
      o.header = 0x80u;
      o.zeros = 0;
      P.out[W.seg] = o;
    }
    return;
  }
  const uint32_t size = 1u << S.logb, mask = size - 1u;
  for (uint32_t i = threadIdx.x; i < size / 4; i += kIdxThreads) tab[i] = 0xffffffffu;
  __syncthreads();
  const uint64_t lo = S.beg + (uint64_t)W.chunk * kIdxChunk;
  const uint64_t hi = lo + kIdxChunk < S.end ? lo + kIdxChunk : S.end;
  // whole dwords of the buffer; the windows of the last 7 positions reach past
  // hi, never past the segment's end (a dword that holds the end may be read:
  // it lies in the buffer's last granule at the latest)
  const uint64_t rend = (S.end + 3u) & ~3ull;
  const uint32_t* g32 = reinterpret_cast<const uint32_t*>(P.g);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t base = (lo & ~3ull) + wave * 256u; base < hi; base += kIdxWaves * 256u) {
    const uint64_t off = base + lane * 4u;
    const uint32_t d0 = off < rend ? g32[off >> 2] : 0u;
    const uint64_t eoff = base + 256u + lane * 4u;
    const uint32_t e = lane < 2 && eoff < rend ? g32[eoff >> 2] : 0u;
    const uint32_t e0 = __shfl(e, 0), e1 = __shfl(e, 1);
    const uint32_t n1 = __shfl_down(d0, 1), n2 = __shfl_down(d0, 2);
    const uint32_t d1 = lane < 63 ? n1 : e0;
    const uint32_t d2 = lane < 62 ? n2 : lane == 62 ? e0 : e1;
    if (base >= lo && base + 256u + 8u <= hi)  // (hi <= S.end) wave-uniform
      hash_four<true>(tab, mask, d0, d1, d2, off, lo, hi, S.end);
    else
      hash_four<false>(tab, mask, d0, d1, d2, off, lo, hi, S.end);
  }
  __syncthreads();
  if (!multi) {
    fold_store(tab, s_red, S.logb, W.seg, S, P);
    return;
  }
  uint32_t* gt = P.glob + (uint64_t)S.glob * (kIdxTable / 4);
  for (uint32_t i = threadIdx.x; i < kIdxTable / 4; i += kIdxThreads) {
    const uint32_t v = tab[i];
    if (v != 0xffffffffu) atomicAnd(&gt[i], v);
  }
}

// a segment of several chunks: its table from global memory, then as above
__global__ __launch_bounds__(kIdxThreads) void idx_fold_kernel(IdxParams P)
{
  __shared__ uint32_t tab[kIdxTable / 4];
  __shared__ uint32_t s_red[kIdxWaves];
  const uint32_t seg = P.gseg[blockIdx.x];
  const IdxSeg S = P.seg[seg];
  if (P.ignore_binary && P.flag[seg]) {
    if (threadIdx.x == 0) {
      IdxOut o;
      o.header = 0x80u;
      o.zeros = 0;
      P.out[seg] = o;
    }
    return;
  }
  const uint32_t* gt = P.glob + (uint64_t)S.glob * (kIdxTable / 4);
  for (uint32_t i = threadIdx.x; i < kIdxTable / 4; i += kIdxThreads) tab[i] = gt[i];
  __syncthreads();
  fold_store(tab, s_red, 16, seg, S, P);
}

// the final tables from their slots to their places in the caller's buffer
__global__ __launch_bounds__(256) void idx_emit_kernel(IdxParams P)
{
  const IdxSeg S = P.seg[blockIdx.x];
  const uint32_t lg = P.out[blockIdx.x].header & 0x1Fu;
  if (!lg) return;
  const uint32_t n16 = (1u << lg) / 16;
  const uint4* src = reinterpret_cast<const uint4*>(P.slots + S.slot);
  uint4* dst = reinterpret_cast<uint4*>(P.dst + P.off[blockIdx.x]);
  for (uint32_t i = threadIdx.x; i < n16; i += 256) dst[i] = src[i];
}

// ---- host
uint64_t idx_env(const char* name, uint64_t dflt)
{
  const char* v = std::getenv(name);
  return v && *v ? std::strtoull(v, nullptr, 0) : dflt;
}

// the largest final table of an n-byte segment, as a log2 (n > 0)
uint32_t slot_log(uint64_t n, uint32_t max_noise)
{
  uint32_t lg = 16;
  while ((1u << lg) > kIdxMin && (uint64_t)(1u << (lg - 1)) * max_noise > 100u * n) --lg;
  return lg;
}

struct IndexWs {
  int dev = -1;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  DevBuf<uint8_t> d_desc, d_slots, d_in, d_tab;
  DevBuf<uint32_t> d_glob;
  PinBuf<uint8_t> h_desc, h_stage;

  hipError_t init()
  {
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    return e;
  }
};

constexpr uint64_t kStagePiece = 16ull << 20;

inline uint64_t up16(uint64_t x) { return (x + 15u) & ~15ull; }

// Segments [s0, s1) of the buffer: flags, tables, folds; header / zeros /
// offsets (from *total on) to the host arrays, and the tables to d_tables while
// they fit.  `bounds` are host values.
int index_group(IndexWs* ws, const uint8_t* dbuf, const uint64_t* bounds, uint32_t s0, uint32_t s1, uint32_t accuracy,
                bool ignore_binary, uint8_t* header, uint32_t* zeros, uint64_t* offset, uint8_t* d_tables,
                uint64_t capacity, uint64_t* total, hipStream_t st)
{
  const uint32_t ng = s1 - s0, max_noise = kMaxNoise[accuracy];
  uint64_t nwork = 0, nglob = 0;
  for (uint32_t s = s0; s < s1; ++s) {
    const uint64_t n = bounds[s + 1] - bounds[s];
    const uint64_t c = n ? (n + kIdxChunk - 1) / kIdxChunk : 0;
    nwork += c;
    nglob += c > 1;
  }
  // descriptors, one block: segments, work, global tables' segments, offsets; out and flags follow on the device
  const uint64_t o_seg = 0, o_work = up16(o_seg + ng * sizeof(IdxSeg)), o_gseg = up16(o_work + nwork * sizeof(IdxWork)),
                 o_off = up16(o_gseg + nglob * 4), o_out = up16(o_off + ng * 8ull), o_flag = up16(o_out + ng * sizeof(IdxOut)),
                 o_end = up16(o_flag + ng * 4ull);
  hipError_t e = ws->d_desc.reserve(o_end, o_end + o_end / 4);
  if (e == hipSuccess) e = ws->h_desc.reserve(o_end, o_end + o_end / 4);
  if (e != hipSuccess) return hip_fail(e, "index descriptors");
  IdxSeg* hs = reinterpret_cast<IdxSeg*>(ws->h_desc.p + o_seg);
  IdxWork* hw = reinterpret_cast<IdxWork*>(ws->h_desc.p + o_work);
  uint32_t* hg = reinterpret_cast<uint32_t*>(ws->h_desc.p + o_gseg);
  uint64_t* hoff = reinterpret_cast<uint64_t*>(ws->h_desc.p + o_off);
  IdxOut* hout = reinterpret_cast<IdxOut*>(ws->h_desc.p + o_out);
  uint64_t slots = 0, iw = 0, ig = 0;
  for (uint32_t k = 0; k < ng; ++k) {
    const uint64_t beg = bounds[s0 + k], end = bounds[s0 + k + 1], n = end - beg;
    IdxSeg& S = hs[k];
    S.beg = beg, S.end = end, S.slot = slots, S.logb = 0, S.glob = kNoGlob;
    if (!n) continue;
    const uint64_t c = (n + kIdxChunk - 1) / kIdxChunk;
    S.logb = c > 1 ? 16 : slot_log(n, max_noise);
    slots += 1ull << S.logb;
    if (c > 1) {
      hg[ig] = k;
      S.glob = (uint32_t)ig++;
    }
    for (uint64_t j = 0; j < c; ++j) hw[iw].seg = k, hw[iw++].chunk = (uint32_t)j;
  }
  if ((e = ws->d_slots.reserve(slots, slots + slots / 4)) != hipSuccess ||
      (e = ws->d_glob.reserve(nglob * (kIdxTable / 4), nglob * (kIdxTable / 4))) != hipSuccess)
    return hip_fail(e, "index tables");
  IdxParams P{};
  P.g = dbuf;
  P.seg = reinterpret_cast<const IdxSeg*>(ws->d_desc.p + o_seg);
  P.work = reinterpret_cast<const IdxWork*>(ws->d_desc.p + o_work);
  P.gseg = reinterpret_cast<const uint32_t*>(ws->d_desc.p + o_gseg);
  P.off = reinterpret_cast<const uint64_t*>(ws->d_desc.p + o_off);
  P.out = reinterpret_cast<IdxOut*>(ws->d_desc.p + o_out);
  P.flag = reinterpret_cast<uint32_t*>(ws->d_desc.p + o_flag);
  P.slots = ws->d_slots;
  P.glob = ws->d_glob;
  P.dst = d_tables;
  P.max_noise = max_noise;
  P.ignore_binary = ignore_binary ? 1u : 0u;
  // (an empty segment gets no workgroup: its out entry is the zero of this memset)
  if ((e = hipMemcpyAsync(ws->d_desc.p, ws->h_desc.p, o_off, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemsetAsync(ws->d_desc.p + o_out, 0, o_end - o_out, st)) != hipSuccess ||
      (nglob && (e = hipMemsetAsync(ws->d_glob.p, 0xff, nglob * kIdxTable, st)) != hipSuccess))
    return hip_fail(e, "index descriptors");
  hipLaunchKernelGGL(idx_flag_kernel, dim3(ng), dim3(kIdxFlagThreads), 0, st, P);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "index flags");
  if (nwork) {
    hipLaunchKernelGGL(idx_hash_kernel, dim3((uint32_t)nwork), dim3(kIdxThreads), 0, st, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "index hash");
  }
  if (nglob) {
    hipLaunchKernelGGL(idx_fold_kernel, dim3((uint32_t)nglob), dim3(kIdxThreads), 0, st, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "index fold");
  }
  if ((e = hipMemcpyAsync(hout, P.out, ng * sizeof(IdxOut), hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "index result copy");
  uint64_t t = *total;
  for (uint32_t k = 0; k < ng; ++k) {
    const uint32_t lg = hout[k].header & 0x1Fu;
    if (lg > hs[k].logb) return fail(UGPU_DEVICE, "index table larger than its bound");
    header[s0 + k] = (uint8_t)hout[k].header;
    zeros[s0 + k] = hout[k].zeros;
    offset[s0 + k] = hoff[k] = t;
    t += lg ? 1ull << lg : 0;
  }
  *total = t;
  if (d_tables && t <= capacity && nwork) {
    if ((e = hipMemcpyAsync(ws->d_desc.p + o_off, hoff, ng * 8ull, hipMemcpyHostToDevice, st)) != hipSuccess)
      return hip_fail(e, "index offsets");
    hipLaunchKernelGGL(idx_emit_kernel, dim3(ng), dim3(256), 0, st, P);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
      return hip_fail(e, "index emit");
  }
  return UGPU_OK;
}

// all segments, in groups whose tables stay inside the workspace bound
int index_segments(IndexWs* ws, const uint8_t* dbuf, const uint64_t* bounds, uint32_t nseg, uint32_t accuracy,
                   bool ignore_binary, uint8_t* header, uint32_t* zeros, uint64_t* offset, uint8_t* d_tables,
                   uint64_t capacity, uint64_t* total, hipStream_t st)
{
  const uint64_t limit = std::max<uint64_t>(idx_env("UGPU_INDEX_WS_BYTES", 256ull << 20), kIdxTable * 2ull);
  const uint32_t max_noise = kMaxNoise[accuracy];
  *total = 0;
  for (uint32_t s = 0; s < nseg;) {
    uint32_t j = s;
    uint64_t bytes = 0, work = 0;
    for (; j < nseg; ++j) {
      const uint64_t n = bounds[j + 1] - bounds[j];
      const uint64_t c = n ? (n + kIdxChunk - 1) / kIdxChunk : 0;
      const uint64_t b = !n ? 0 : c > 1 ? 2ull * kIdxTable : 1ull << slot_log(n, max_noise);
      if (j > s && (bytes + b > limit || work + c > 0x7fffffffull)) break;
      bytes += b;
      work += c;
    }
    if (work > 0x7fffffffull) return fail(UGPU_INVAL, "segment too large");
    const int rc = index_group(ws, dbuf, bounds, s, j, accuracy, ignore_binary, header, zeros, offset, d_tables, capacity,
                               total, st);
    if (rc) return rc;
    s = j;
  }
  offset[nseg] = *total;
  return UGPU_OK;
}

}  // namespace

}  // namespace ugpu

// ---------------------------------------------------------------- C ABI
using namespace ugpu;

extern "C" {

uint64_t ugpu_index_chunk(void) { return kIdxChunk; }

int ugpu_index_tables(const uint8_t* dbuf, uint64_t len, const uint64_t* bounds, uint32_t nseg, uint32_t accuracy,
                      uint32_t flags, uint8_t* header, uint32_t* zero_bits, uint64_t* offset, uint8_t* d_tables,
                      uint64_t capacity, uint64_t* tables_len, void* stream)
{
  if (accuracy > 9) return fail(UGPU_INVAL, "accuracy is 0..9");
  if (flags & ~(uint32_t)UGPU_INDEX_IGNORE_BINARY) return fail(UGPU_INVAL, "unknown flag");
  if (!bounds || !offset || !tables_len || (nseg && (!dbuf || !header || !zero_bits)))
    return fail(UGPU_INVAL, "NULL argument");
  if ((reinterpret_cast<uintptr_t>(dbuf) | reinterpret_cast<uintptr_t>(d_tables)) & 15u)
    return fail(UGPU_INVAL, "buffers must be 16-byte aligned");
  for (uint32_t s = 0; s < nseg; ++s)
    if (bounds[s] > bounds[s + 1]) return fail(UGPU_INVAL, "bounds must ascend");
  if (bounds[nseg] > len) return fail(UGPU_INVAL, "bounds pass the buffer");
  *tables_len = 0;
  offset[0] = 0;
  if (!nseg) return UGPU_OK;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  WsLease<IndexWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "index workspace");
  const int rc = index_segments(ws.ws, dbuf, bounds, nseg, accuracy, (flags & UGPU_INDEX_IGNORE_BINARY) != 0, header,
                                zero_bits, offset, d_tables, capacity, tables_len, reinterpret_cast<hipStream_t>(stream));
  if (rc) return rc;
  if (d_tables && *tables_len > capacity) return fail(UGPU_CAPACITY, "index tables do not fit");
  return UGPU_OK;
}

int ugpu_index_free(ugpu_index_result* r)
{
  if (!r) return UGPU_OK;
  std::free(r->header);
  std::free(r->zero_bits);
  std::free(r->offset);
  std::free(r->tables);
  std::free(r);
  return UGPU_OK;
}

}  // extern "C"

namespace {

// inputs [i0, i1) (`total` bytes, > 0) back to back into ws->d_in, in pieces
// through the two halves of the pinned stage
int index_upload(IndexWs* ws, const uint8_t* const* bufs, const uint64_t* lens, uint32_t i0, uint32_t i1, uint64_t total)
{
  hipError_t e = ws->d_in.reserve(total, total + total / 8, 32);
  if (e == hipSuccess) e = ws->h_stage.reserve(2 * kStagePiece, 2 * kStagePiece);
  if (e != hipSuccess) return hip_fail(e, "index input buffers");
  if ((e = hipMemsetAsync(ws->d_in.p + total, 0, 32, ws->st)) != hipSuccess) return hip_fail(e, "index input");
  uint32_t i = i0;
  uint64_t in_off = 0;  // bytes of input i already taken
  uint32_t piece = 0;
  for (uint64_t done = 0; done < total; ++piece) {
    const uint64_t m = std::min(kStagePiece, total - done);
    uint8_t* h = ws->h_stage.p + (piece & 1u) * kStagePiece;
    if (piece >= 2 && (e = hipEventSynchronize(ws->ev[piece & 1u])) != hipSuccess) return hip_fail(e, "index input");
    for (uint64_t f = 0; f < m;) {
      while (in_off == lens[i]) ++i, in_off = 0;  // (i < i1: the bytes left are theirs)
      const uint64_t c = std::min(m - f, lens[i] - in_off);
      std::memcpy(h + f, bufs[i] + in_off, c);
      f += c;
      in_off += c;
    }
    if ((e = hipMemcpyAsync(ws->d_in.p + done, h, m, hipMemcpyHostToDevice, ws->st)) != hipSuccess ||
        (e = hipEventRecord(ws->ev[piece & 1u], ws->st)) != hipSuccess)
      return hip_fail(e, "index input copy");
    done += m;
  }
  (void)i1;
  return UGPU_OK;
}

template <class T>
bool index_grow(T*& a, uint64_t n)
{
  void* p = std::realloc(a, (n ? n : 1) * sizeof(T));
  if (!p) return false;
  a = static_cast<T*>(p);
  return true;
}

}  // namespace

extern "C" int ugpu_index_batch(const uint8_t* const* bufs, const uint64_t* lens, uint32_t ninputs, uint32_t accuracy,
                                uint32_t flags, ugpu_index_result** out)
{
  if (!out || (ninputs && (!bufs || !lens))) return fail(UGPU_INVAL, "NULL argument");
  *out = nullptr;
  if (accuracy > 9) return fail(UGPU_INVAL, "accuracy is 0..9");
  if (flags & ~(uint32_t)UGPU_INDEX_IGNORE_BINARY) return fail(UGPU_INVAL, "unknown flag");
  for (uint32_t i = 0; i < ninputs; ++i)
    if (!bufs[i] && lens[i]) return fail(UGPU_INVAL, "NULL input with a length");
  ugpu_index_result* r = static_cast<ugpu_index_result*>(std::calloc(1, sizeof(ugpu_index_result)));
  if (!r) return fail(UGPU_NOMEM, "host allocation");
  r->ninputs = ninputs;
  r->accuracy = accuracy;
  r->header = static_cast<uint8_t*>(std::calloc((uint64_t)ninputs + 1, 1));
  r->zero_bits = static_cast<uint32_t*>(std::calloc((uint64_t)ninputs + 1, 4));
  r->offset = static_cast<uint64_t*>(std::calloc((uint64_t)ninputs + 1, 8));
  if (!r->header || !r->zero_bits || !r->offset) {
    ugpu_index_free(r);
    return fail(UGPU_NOMEM, "host allocation");
  }
  const uint64_t limit = std::max<uint64_t>(idx_env("UGPU_BATCH_BYTES", 1ull << 30), 1);
  const uint32_t max_noise = kMaxNoise[accuracy];
  IndexWs* ws = nullptr;
  std::vector<uint64_t> bounds;
  int rc = UGPU_OK;
  uint64_t have = 0;  // bytes of r->tables
  for (uint32_t i = 0; i < ninputs && !rc;) {
    // the next sub-batch: cut only between inputs, a larger input by itself
    uint32_t j = i;
    uint64_t total = 0, tabs = 0;
    for (; j < ninputs; ++j) {
      if (j > i && total + lens[j] > limit) break;
      total += lens[j];
      tabs += lens[j] ? 1ull << slot_log(lens[j], max_noise) : 0;
    }
    if (!total) {  // empty inputs only
      for (uint32_t k = i; k < j; ++k) r->offset[k] = have;
      i = j;
      continue;
    }
    if (!ws) {
      int dev = 0;
      const hipError_t e = hipGetDevice(&dev);
      if (e != hipSuccess) rc = hip_fail(e, "hipGetDevice");
      if (!rc && !(ws = WsLease<IndexWs>::take(dev))) rc = fail(UGPU_NOMEM, "index workspace");
      if (rc) break;
    }
    const uint32_t nseg = j - i;
    bounds.resize((size_t)nseg + 1);
    bounds[0] = 0;
    for (uint32_t k = 0; k < nseg; ++k) bounds[k + 1] = bounds[k] + lens[i + k];
    rc = index_upload(ws, bufs, lens, i, j, total);
    hipError_t e = hipSuccess;
    if (!rc && (e = ws->d_tab.reserve(tabs, tabs + tabs / 4)) != hipSuccess) rc = hip_fail(e, "index tables");
    uint64_t got = 0;
    std::vector<uint64_t> off((size_t)nseg + 1);
    if (!rc)
      rc = index_segments(ws, ws->d_in, bounds.data(), nseg, accuracy, (flags & UGPU_INDEX_IGNORE_BINARY) != 0,
                          r->header + i, r->zero_bits + i, off.data(), ws->d_tab, tabs, &got, ws->st);
    if (!rc && got > tabs) rc = fail(UGPU_DEVICE, "index tables pass their bound");
    if (!rc && !index_grow(r->tables, have + got)) rc = fail(UGPU_NOMEM, "index tables");
    if (!rc && got &&
        ((e = hipMemcpyAsync(r->tables + have, ws->d_tab.p, got, hipMemcpyDeviceToHost, ws->st)) != hipSuccess ||
         (e = hipStreamSynchronize(ws->st)) != hipSuccess))
      rc = hip_fail(e, "index tables copy");
    for (uint32_t k = 0; k < nseg; ++k) r->offset[i + k] = have + off[k];
    have += got;
    i = j;
  }
  if (ws) {
    (void)hipStreamSynchronize(ws->st);
    WsLease<IndexWs>::give(ws);
  }
  if (rc) {
    ugpu_index_free(r);
    return rc;
  }
  r->offset[ninputs] = have;
  *out = r;
  return UGPU_OK;
}
