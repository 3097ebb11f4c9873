// ngram_kernel.hip -- FIND behind an n-gram candidate filter (kernel 7), for
// class and wide tables: large string sets (-f words.txt, long alternations),
// whose first bytes cover the alphabet, so that sparse_kernel's byte-set
// prefilter passes everything, and whose tables are too big for its byte format.
//
// A position p can start a match only if its next n bytes (n = 2..4, at most
// the shortest match) are one of the n-byte strings that begin a match.  The
// host hashes those strings into a bitmap of 2^k bits (ngram.hpp, tables.cpp
// build_ngram); the kernel keeps the bitmap in LDS and
//
//   * streams its wave's range in 4 KiB tiles, 16 B per lane and 1 KiB chunk,
//     by non-temporal buffer loads into two register sets used in turn;
//   * builds the n-byte window of each of a lane's 16 positions (the last
//     n - 1 need the first bytes of the next lane's granule, of the next chunk
//     or of the next tile), hashes it and gathers its bit from the bitmap: one
//     LDS dword per position, spread over the banks by the hash;
//   * queues the candidates in position order in a per-wave list; when 64 are
//     queued each lane walks one (walk<FMT, W>: the plain or the option-W
//     walk), and the FIND chain over them is the greedy rule "keep c iff
//     c >= the end of the last kept match", resolved in order from the lanes'
//     results.  The rule is exact: a position that is no candidate starts no
//     match, so the chain only steps p + 1 over it, and a candidate whose walk
//     fails (also by the W rules) steps p + 1 as well.
//
// A window must lie inside the readable bytes: a position within n - 1 bytes
// of the readable end is no candidate at the end of the stream (a match has at
// least n bytes) and always one before it (its walk reports HALO, as without
// the filter).  Nothing depends on what the loads return past the readable end.
//
// Records are wfind_kernel's: one BlockRec per wave, speculative entry at the
// range start, stitched by fix_kernel; the WRITE pass repeats the scan from
// the record's exact entry and writes at its output base.  The main loop has
// no workgroup barrier (one after staging the tables).
//
// A long run of overlapping candidates (aaaa... against a set holding aaaa)
// costs one walk of a few bytes per position and at most 64 chain steps per
// batch: bounded by the input length.
#include "device_common.hpp"
#include "ngram.hpp"

namespace ugpu {

namespace {

constexpr int kNgWaves = 8;            // waves (records) per workgroup: one staged bitmap
constexpr uint32_t kNgBatch = 64;      // candidates per walk batch
constexpr size_t kNgLdsBudget = 64 * 1024;

// LDS image: bitmap (2^k bits), Word ranges (option W; 2 x u32 each), class
// bytes (256), the per-wave candidate lists (u32 offsets from the wave's first
// tile), then the class table (u16) when it fits (tab_lds)
__host__ __device__ inline size_t ngram_smem(uint32_t ng_log2, uint32_t nwtab, uint32_t ntrans_pad, bool tab_lds)
{
  return ((size_t)1 << (ng_log2 - 3)) + 8 * (size_t)nwtab + 256 + (size_t)kNgWaves * kNgBatch * 4 +
         (tab_lds ? 2 * (size_t)ntrans_pad : 0);
}

struct TileLoad {
  __amdgpu_buffer_rsrc_t rs;
};

// (sparse_kernel.hip stream16: 16-byte granules wholly past the resource's
// bytes read as 0 and touch no memory)
__device__ __forceinline__ uint4 stream16(const TileLoad& L, uint32_t off)
{
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  const v4u v = __builtin_amdgcn_raw_buffer_load_b128(L.rs, (int)off, 0, 2 /* nt */);
  return uint4{v.x, v.y, v.z, v.w};
}

// Buffer resource of tile i of a wave (base = the wave's first tile, rel =
// loadable bytes from there: a multiple of 16, < 2^32)
__device__ __forceinline__ TileLoad wave_tile(const uint8_t* wbase, uint32_t i, uint32_t rel)
{
  const uint32_t off = i * (uint32_t)kWaveTile;
  const uint32_t n = rel > off ? rel - off : 0u;
  const int nr = __builtin_amdgcn_readfirstlane((int)(n < (uint32_t)kWaveTile ? n : (uint32_t)kWaveTile));
  return TileLoad{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(wbase + off), (short)0, nr, 0x00020000)};
}

// the first four bytes of a tile (0 past the loadable bytes), the same for all lanes
__device__ __forceinline__ uint32_t first_dword(const TileLoad& L)
{
  return __builtin_amdgcn_raw_buffer_load_b32(L.rs, 0, 0, 0);
}

__device__ __forceinline__ void wave_lds_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the chain state of a wave (uniform), its sums (per lane) and its list
struct NgWave {
  uint64_t x;        // the chain's next position: the end of the last kept match (or the entry)
  uint64_t widx;     // WRITE: index of the next record
  uint32_t dn;       // queued candidates
  uint32_t ovf, wover;
  CountEm acc;
};

// the 16 filter bits of a lane's granule d0..d3 (d4 = the four bytes after it)
__device__ __forceinline__ uint32_t ngram_bits16(const uint32_t* bm, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3,
                                                 uint32_t d4, uint32_t mask, uint32_t k)
{
  const uint32_t d[5] = {d0, d1, d2, d3, d4};
  uint32_t mk = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t lo = d[j >> 2], hi = d[(j >> 2) + 1];
    const uint32_t win = (j & 3) ? __builtin_amdgcn_alignbit(hi, lo, 8 * (j & 3)) : lo;
    mk |= (ngram_test(bm, win & mask, k) ? 1u : 0u) << j;
  }
  return mk;
}

// walk the queued candidates (one per lane) and run the chain over them
template <int FMT, bool WRITE, int M>
__device__ __forceinline__ void ngram_flush(const uint32_t* list, int lane, uint64_t wb, const Tab<FMT>& T, const Win& w,
                                            const Ctx& C, const ScanParams& P, NgWave& st)
{
  wave_lds_sync();  // the list writes of all lanes
  const bool have = (uint32_t)lane < st.dn;
  const uint64_t c = have ? wb + list[lane] : ~0ull;
  uint32_t le = 0;
  uint64_t len = 0;
  if (have && c >= st.x) len = walk<FMT, M>(T, w, c, le, st.ovf);
  uint64_t m = __ballot(len != 0);
  while (m) {
    const int f = __builtin_ctzll(m);
    m &= m - 1;
    const uint64_t cf = __shfl(c, f, 64), lf = __shfl(len, f, 64);
    if (cf < st.x) continue;  // inside the match kept before it
    if (lane == f) {
      if constexpr (WRITE) {
        WriteEm em{st.widx, P.out_capacity, P.out_start, P.out_len, P.out_cap};
        em.put(C, c, len, le, +1);
        st.wover |= em.overflow;
      } else {
        st.acc.put(C, c, len, le, +1);
      }
    }
    ++st.widx;
    st.x = cf + lf;
  }
  st.dn = 0;
  wave_lds_sync();  // the list is free again
}

// one tile: filter, queue, flush full batches
template <int FMT, bool WRITE, int M>
__device__ __forceinline__ void ngram_tile(const uint4 (&a)[4], uint32_t nfirst, uint64_t ts, uint64_t wlo, uint64_t whi,
                                           int lane, const uint32_t* bm, uint32_t* list, uint64_t wb, const Tab<FMT>& T,
                                           const Win& w, const Ctx& C, const ScanParams& P, NgWave& st)
{
  const uint32_t mask = ngram_mask(P.ng_n);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 v = a[k];
    // the four bytes after the lane's granule: the next lane's, the next chunk's or the next tile's
    uint32_t d4 = __shfl_down(v.x, 1, 64);
    const uint32_t nx = k < 3 ? __shfl(a[k < 3 ? k + 1 : 3].x, 0, 64) : nfirst;
    if (lane == 63) d4 = nx;
    uint32_t mk = ngram_bits16(bm, v.x, v.y, v.z, v.w, d4, mask, P.ng_log2);
    const uint64_t p0 = ts + 1024u * k + 16u * lane;
    // windows that reach past the readable end: no candidates at the end of
    // the stream, candidates before it (the next bytes are not read yet)
    if (p0 + 15 + P.ng_n > P.rend) {
      const uint64_t full = P.rend >= p0 + P.ng_n ? P.rend - P.ng_n + 1 - p0 : 0;  // positions with a whole window
      const uint64_t rd = P.rend > p0 ? P.rend - p0 : 0;                          // readable positions
      mk &= (uint32_t)lowbits(full < 16 ? full : 16);
      if (!P.at_eof) mk |= (uint32_t)(lowbits(rd < 16 ? rd : 16) & ~lowbits(full < 16 ? full : 16));
    }
    // the wave's range, and the positions the chain has already passed
    const uint64_t lo = wlo > st.x ? wlo : st.x;
    if (lo > p0) mk &= (uint32_t)~lowbits(lo - p0 < 16 ? lo - p0 : 16);
    mk &= (uint32_t)lowbits(whi > p0 ? (whi - p0 < 16 ? whi - p0 : 16) : 0);
    mk &= 0xffffu;
    if (!__ballot(mk != 0)) continue;
    // rank the chunk's candidates in position order
    const uint32_t cnt = __popc(mk);
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    const uint32_t tot = __shfl(incl, 63, 64);
    const uint32_t rank = incl - cnt;
    const uint32_t rel = (uint32_t)(p0 - wb);
    for (uint32_t done = 0; done < tot;) {
      if (st.dn == kNgBatch) ngram_flush<FMT, WRITE, M>(list, lane, wb, T, w, C, P, st);
      const uint32_t take = tot - done < kNgBatch - st.dn ? tot - done : kNgBatch - st.dn;
      uint32_t m = mk, r = rank;
      while (m) {
        const uint32_t bit = __builtin_ctz(m);
        m &= m - 1;
        if (r >= done && r - done < take) list[st.dn + r - done] = rel + bit;
        ++r;
      }
      st.dn += take;
      done += take;
    }
  }
}

template <int FMT, bool WRITE, int M, bool TLDS>
__global__ __launch_bounds__(kNgWaves * 64) void ngram_kernel(ScanParams P)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t nsm[];
  const uint32_t bm_words = 1u << (P.ng_log2 - 5);
  const uint32_t nwt = M == kWalkWord ? P.nwtab : 0u;
  uint32_t* s_bm = reinterpret_cast<uint32_t*>(nsm);
  uint32_t* s_wtab = s_bm + bm_words;
  uint8_t* s_cls = reinterpret_cast<uint8_t*>(s_wtab + 2 * nwt);
  uint32_t* s_list = reinterpret_cast<uint32_t*>(s_cls + 256);
  uint16_t* s_trans = reinterpret_cast<uint16_t*>(s_list + kNgWaves * kNgBatch);
  for (uint32_t i = threadIdx.x; i < bm_words; i += blockDim.x) s_bm[i] = P.ng_bitmap[i];
  for (uint32_t i = threadIdx.x; i < 2 * nwt; i += blockDim.x) s_wtab[i] = P.wtab[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) s_cls[i] = P.cls[i];
  if constexpr (TLDS)
    for (uint32_t i = threadIdx.x; i < P.ntrans_pad; i += blockDim.x) s_trans[i] = P.trans[i];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t r = (uint64_t)blockIdx.x * kNgWaves + wid;
  if (r >= P.nrec) return;  // wave-uniform
  uint64_t tb = P.t0 + r * P.tpb;
  uint64_t te = tb + P.tpb < P.t1 ? tb + P.tpb : P.t1;
  if (tb > te) tb = te;
  const uint64_t wlo = clampu(tb * P.unit, P.lo, P.hi);
  const uint64_t whi = clampu(te * P.unit, P.lo, P.hi);
  Tab<FMT> T;
  if constexpr (FMT == 2)
    T = Tab<2>{P.trans32, s_cls, P.start, P.accb};
  else
    T = Tab<FMT>{TLDS ? s_trans : P.trans, s_cls, P.start, P.accb};
  const Ctx C{P.caps, P.log_row, P.delta};
  Win w = win_of(P);
  w.wtab = s_wtab;
  w.caps = nullptr;  // (no REDO accepts on this kernel: plan_ngram)
  uint32_t* list = s_list + wid * kNgBatch;

  NgWave st;
  st.x = WRITE ? P.entries[r] : wlo;
  if (st.x < wlo) st.x = wlo;
  st.widx = WRITE ? P.out_base[r] : 0;
  st.dn = 0;
  st.ovf = st.wover = 0;

  if (whi > wlo) {
    // tiles [tb, te), and the first granule after them (the windows of the
    // last positions); all loop control is 32-bit (a record has < 2^30 bytes)
    const uint32_t n = (uint32_t)(te - tb);
    const uint64_t wb = tb * kWaveTile;
    const uint8_t* wbase = P.g + wb;
    const uint64_t rend16 = (P.rend + 15) & ~uint64_t(15);
    const uint64_t relw = rend16 > wb ? rend16 - wb : 0;
    const uint64_t span = (uint64_t)n * kWaveTile + 16;
    const uint32_t rel = (uint32_t)(relw < span ? relw : span);
    const uint32_t lo16 = 16u * lane;
    // Two register sets used in turn (a = tile i, b = tile i + 1): a set is
    // loaded while the other one is filtered.  A tile's last windows need the
    // first dword of the tile after it, which is loaded (one dword, the same
    // for all lanes) a step ahead of that tile, so no step waits for the
    // loads it has just issued.
    uint4 a[4], b[4];
    uint32_t nfa, nfb;  // the first dword of the tile after a / after b
    {
      const TileLoad La = wave_tile(wbase, 0, rel);
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = stream16(La, lo16 + 1024u * k);
      nfa = first_dword(wave_tile(wbase, 1, rel));
    }
    for (uint32_t i = 0; i < n; i += 2) {
      {
        const TileLoad L = wave_tile(wbase, i + 1, rel);
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = stream16(L, lo16 + 1024u * k);
        nfb = first_dword(wave_tile(wbase, i + 2, rel));
      }
      ngram_tile<FMT, WRITE, M>(a, nfa, wb + (uint64_t)i * kWaveTile, wlo, whi, lane, s_bm, list, wb, T, w, C, P, st);
      {
        const TileLoad L = wave_tile(wbase, i + 2, rel);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = stream16(L, lo16 + 1024u * k);
        nfa = first_dword(wave_tile(wbase, i + 3, rel));
      }
      if (i + 1 < n)
        ngram_tile<FMT, WRITE, M>(b, nfb, wb + (uint64_t)(i + 1) * kWaveTile, wlo, whi, lane, s_bm, list, wb, T, w, C, P,
                                  st);
    }
    if (st.dn) ngram_flush<FMT, WRITE, M>(list, lane, wb, T, w, C, P, st);
  }

  if constexpr (WRITE) {
    if (st.wover) atomicOr(P.flags, UGPU_FLAG_CAPACITY);
  } else {
    const uint64_t c = wave_sum(st.acc.cnt), d = wave_sum(st.acc.dg), dc = wave_sum(st.acc.dc);
    if (lane == 0) {
      BlockRec rec;
      rec.entry = wlo;
      rec.exit = whi > wlo ? (st.x > whi ? st.x : whi) : wlo;
      rec.cnt = c;
      rec.dg = d;
      rec.dc = dc;
      rec.pad0 = rec.pad1 = rec.pad2 = 0;
      P.recs[r] = rec;
    }
  }
  if (__ballot(st.ovf != 0) && lane == 0) atomicOr(P.flags, UGPU_FLAG_HALO);
}

template <int FMT, bool WRITE, int M, bool TLDS>
hipError_t ngram_one(const ScanParams& P, hipStream_t stream)
{
  const size_t smem = ngram_smem(P.ng_log2, M == kWalkWord ? P.nwtab : 0u, P.ntrans_pad, TLDS);
  hipLaunchKernelGGL((ngram_kernel<FMT, WRITE, M, TLDS>), dim3(P.grid), dim3(kNgWaves * 64), smem, stream, P);
  return hipGetLastError();
}

template <int FMT, int M>
hipError_t ngram_fmt(const ScanParams& P, bool write, hipStream_t stream)
{
  if constexpr (FMT == 1) {
    if (P.ng_tab_lds) return write ? ngram_one<1, true, M, true>(P, stream) : ngram_one<1, false, M, true>(P, stream);
  }
  return write ? ngram_one<FMT, true, M, false>(P, stream) : ngram_one<FMT, false, M, false>(P, stream);
}

}  // namespace

uint32_t ngram_waves() { return kNgWaves; }

// a class table sits in LDS beside the bitmap when the whole image stays within kNgLdsBudget
bool ngram_tab_lds(uint32_t format, uint32_t ntrans_pad, uint32_t nwtab, uint32_t ng_log2)
{
  return format == 1 && ngram_smem(ng_log2, nwtab, ntrans_pad, true) <= kNgLdsBudget;
}

hipError_t launch_ngram(const ScanParams& P, uint32_t format, bool write, hipStream_t stream)
{
  if (!P.ng_bitmap || P.ng_n < 2 || P.ng_n > kNgMaxN || P.ng_log2 < kNgMinLog2 || P.ng_log2 > kNgMaxLog2 || format == 0 ||
      P.unit != (uint32_t)kWaveTile)
    return hipErrorInvalidValue;
  if (ngram_smem(P.ng_log2, P.nwtab, P.ntrans_pad, P.ng_tab_lds != 0) > kNgLdsBudget) return hipErrorInvalidValue;
  if (P.wtab) return format == 1 ? ngram_fmt<1, kWalkWord>(P, write, stream) : ngram_fmt<2, kWalkWord>(P, write, stream);
  return format == 1 ? ngram_fmt<1, kWalkPlain>(P, write, stream) : ngram_fmt<2, kWalkPlain>(P, write, stream);
}

}  // namespace ugpu
