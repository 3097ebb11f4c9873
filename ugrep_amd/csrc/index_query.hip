// index_query.hip -- the index query on the device: ugpu_index_query and
// ugpu_index_query_store (include/ugpu.h), i.e. Pattern::match_hfa
// (lib/pattern.cpp:4757-4815) and the per-record decision of
// src/ugrep.cpp:10060-10099 over the records ugpu_index_tables leaves.
//
// One wave walks one record, kQWaves waves to a workgroup; no workgroup
// barrier is used, so a wave leaves as soon as its record is decided.  Levels
// run in order.  Within a level the lanes take (entry, offset) pairs, eight
// entries by eight offsets at a time: a lane walks the hash ranges of its pair
// and probes min(hi - lo + 1, size) slots of a range (a range as long as the
// table meets every slot).  A range of more than kQShort slots is handed to
// the whole wave, 64 slots a step, so that \w+ over a 64 KiB table is not one
// lane's walk.  A ballot gives "this (entry, offset) passed", its byte per
// entry "the first offset passed" (the entry marks its successors, or, dead,
// ends the query with keep) and "all offsets passed" (the level goes on).  The
// two visit sets of 1024 bits lie in LDS per wave and are never cleared, as in
// the reference.
//
// The table: up to `stage` bytes it is copied into the wave's LDS first, a
// larger one is probed in global memory.  profiles/index_query_bench.json
// holds the measurement behind kQSwitch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hfa.hpp"
#include "hip_host.hpp"

namespace ugpu {

namespace {

constexpr uint32_t kQWaves = 4;        // records per workgroup
constexpr uint32_t kQStage = 4096;     // bytes of LDS per wave for a staged table: the most that costs no occupancy
constexpr uint32_t kQSwitch = 2048;    // the default switch: a larger table is probed in global memory (measured)
constexpr uint32_t kQWavesAll = 2;     // UGPU_QUERY_FORCE_LDS: every table staged, 64 KiB per wave
constexpr uint32_t kQStageAll = 65536;
constexpr uint32_t kQShort = 8;        // slots of a range one lane probes by itself
constexpr uint8_t kMagic[5] = {'U', 'G', '#', 3, 0};

struct QParams {
  const uint32_t* w;  // the automaton's words
  HfaView v;
  const uint8_t* tables;
  const uint64_t* off;
  const uint8_t* header;
  uint8_t* keep;
  uint32_t nrec, flags, stage;
};

template <uint32_t WAVES, uint32_t STAGE>
__global__ __launch_bounds__(WAVES * 64) void index_query_kernel(QParams P)
{
  __shared__ uint4 s_tab[WAVES][STAGE / 16];
  __shared__ uint32_t s_vis[WAVES][2][kHfaStates / 32];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t rec = blockIdx.x * WAVES + wave;
  if (rec >= P.nrec) return;
  const uint32_t b = P.header[rec], lg = b & 0x1Fu;
  // src/ugrep.cpp:10060-10099
  const bool skip = ((b & 0x80u) && (P.flags & UGPU_QUERY_IGNORE_BINARY)) || ((b & 0x60u) && !(P.flags & UGPU_QUERY_DECOMPRESS));
  if (skip || !lg) {  // (without a table: an empty file is skipped, a binary one kept)
    if (lane == 0) P.keep[rec] = !skip && (b & 0x80u) ? 1 : 0;
    return;
  }
  const uint32_t size = 1u << lg, mask = size - 1;
  const uint8_t* gtab = P.tables + P.off[rec];
  const bool staged = size <= P.stage && size <= STAGE;
  const uint8_t* ltab = reinterpret_cast<const uint8_t*>(s_tab[wave]);
  if (staged) {
    const uint4* src = reinterpret_cast<const uint4*>(gtab);
    for (uint32_t i = lane; i < size / 16; i += 64) s_tab[wave][i] = src[i];
  }
  uint32_t(*vis)[kHfaStates / 32] = s_vis[wave];
  vis[lane >> 5][lane & 31u] = 0;
  __threadfence_block();
  auto probe = [&](uint32_t h) -> uint32_t { return staged ? ltab[h & mask] : gtab[h & mask]; };

  const uint32_t* w = P.w;
  const HfaView& v = P.v;
  const uint32_t el = lane >> 3, k = lane & 7u;
  uint32_t keep = 1;
  for (uint32_t level = 0; level < kHfaDepth; ++level) {
    const uint32_t e0 = w[v.level_first + level], e1 = w[v.level_first + level + 1];
    const uint32_t npair = (level < kHfaChain ? level : kHfaChain - 1) + 1;
    const uint32_t* cur = vis[level & 1u];
    uint32_t* nxt = vis[~level & 1u];
    bool any = false, accept = false;
    for (uint32_t base = e0; base < e1 && !accept; base += 8) {
      const uint32_t e = base + el;
      const bool in = e < e1;
      bool on = in && k < npair;
      if (on && level) {
        const uint32_t st = w[v.entry_state + e];
        on = (cur[st >> 5] >> (st & 31u)) & 1u;
      }
      const uint32_t bit = 1u << (npair - 1 - (k < npair ? k : 0));
      uint32_t r = 0, r1 = 0;
      if (on) {
        const uint32_t p = w[v.entry_pair + e] + k;
        r = w[v.pair_range + p], r1 = w[v.pair_range + p + 1];
      }
      bool flag = false;
      for (;; ++r) {
        const bool has = on && !flag && r < r1;
        if (!__ballot(has)) break;
        uint32_t lo = 0, n = 0;
        if (has) {
          const uint32_t x = w[v.range + r];
          lo = x & 0xFFFFu;
          n = min((x >> 16) - lo + 1, size);
          if (n <= kQShort)
            for (uint32_t i = 0; i < n && !flag; ++i) flag = !(probe(lo + i) & bit);
        }
        for (uint64_t m = __ballot(has && n > kQShort); m; m &= m - 1) {
          const int src = __ffsll((long long)m) - 1;
          const uint32_t blo = (uint32_t)__shfl((int)lo, src, 64), bn = (uint32_t)__shfl((int)n, src, 64),
                         bbit = (uint32_t)__shfl((int)bit, src, 64);
          bool found = false;
          for (uint32_t i0 = 0; i0 < bn && !found; i0 += 64) {
            const uint32_t i = i0 + lane;
            found = __ballot(i < bn && !(probe(blo + i) & bbit)) != 0;
          }
          if ((int)lane == src) flag = found;
        }
      }
      const uint32_t byte = (uint32_t)(__ballot(flag) >> (8 * el)) & 0xFFu;
      const bool first = byte & 1u, all = byte == (1u << npair) - 1;
      const bool dead = in && first && w[v.entry_dead + e];
      accept = __ballot(dead) != 0;
      any = any || __ballot(all) != 0;
      if (in && first && !accept)
        for (uint32_t s = w[v.entry_succ + e] + k; s < w[v.entry_succ + e + 1]; s += 8) {
          const uint32_t st = w[v.succ + s];
          atomicOr(&nxt[st >> 5], 1u << (st & 31u));
        }
    }
    if (accept) break;
    if (!any) {
      keep = 0;
      break;
    }
    __threadfence_block();
  }
  if (lane == 0) P.keep[rec] = (uint8_t)keep;
}

uint64_t q_env(const char* name, uint64_t dflt)
{
  const char* s = std::getenv(name);
  return s && *s ? std::strtoull(s, nullptr, 0) : dflt;
}

uint32_t default_stage() { return (uint32_t)std::min<uint64_t>(q_env("UGPU_QUERY_LDS_BYTES", kQSwitch), kQStage); }

struct QueryWs {
  int dev = -1;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipEvent_t tm[2] = {nullptr, nullptr};  // around the kernel (ugpu_index_query_kernel_ms)
  uint64_t hfa_id = 0;  // the automaton d_hfa holds
  DevBuf<uint32_t> d_hfa;
  DevBuf<uint8_t> d_desc, d_tab;
  PinBuf<uint8_t> h_desc, h_stage;

  hipError_t init()
  {
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreate(&tm[i]);
    return e;
  }
};

thread_local float g_query_kernel_ms = 0.f;  // the kernels of this thread's last call

constexpr uint64_t kStagePiece = 16ull << 20;
inline uint64_t up16(uint64_t x) { return (x + 15u) & ~15ull; }

const uint32_t kQueryFlags = UGPU_QUERY_IGNORE_BINARY | UGPU_QUERY_DECOMPRESS | UGPU_QUERY_FORCE_LDS | UGPU_QUERY_FORCE_GLOBAL;

// every table inside [0, offset[nrec]) at a 16-byte aligned place
int check_records(const uint8_t* header, const uint64_t* offset, uint32_t nrec)
{
  for (uint32_t s = 0; s < nrec; ++s) {
    const uint32_t lg = header[s] & 0x1Fu;
    if (!lg) continue;
    if (lg < 7 || lg > 16) return fail(UGPU_INVAL, "a table has 128 to 65536 bytes");
    if ((offset[s] & 15u) || offset[s] > offset[nrec] || (1ull << lg) > offset[nrec] - offset[s])
      return fail(UGPU_INVAL, "a table lies outside the tables or is not 16-byte aligned");
  }
  return UGPU_OK;
}

// the query over nrec checked records whose tables lie in d_tables; keep: host
int query_records(QueryWs* ws, const ugpu_hfa* hfa, const uint8_t* d_tables, const uint8_t* header, const uint64_t* offset,
                  uint32_t nrec, uint32_t flags, uint8_t* keep, hipStream_t st)
{
  hipError_t e = hipSuccess;
  if (ws->hfa_id != hfa->id) {  // (uploaded once while this workspace serves the same automaton)
    ws->hfa_id = 0;
    const uint64_t n = hfa->words.size();
    if ((e = ws->d_hfa.reserve(n, n + n / 4)) != hipSuccess ||
        (e = hipMemcpyAsync(ws->d_hfa.p, hfa->words.data(), n * 4, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
      return hip_fail(e, "index query automaton");
    ws->hfa_id = hfa->id;
  }
  const uint64_t o_off = 0, o_hdr = up16(8ull * nrec), o_keep = up16(o_hdr + nrec), o_end = up16(o_keep + nrec);
  if ((e = ws->d_desc.reserve(o_end, o_end + o_end / 4)) != hipSuccess ||
      (e = ws->h_desc.reserve(o_end, o_end + o_end / 4)) != hipSuccess)
    return hip_fail(e, "index query descriptors");
  std::memcpy(ws->h_desc.p + o_off, offset, 8ull * nrec);
  std::memcpy(ws->h_desc.p + o_hdr, header, nrec);
  if ((e = hipMemcpyAsync(ws->d_desc.p, ws->h_desc.p, o_keep, hipMemcpyHostToDevice, st)) != hipSuccess)
    return hip_fail(e, "index query descriptors");
  QParams P{};
  P.w = ws->d_hfa;
  P.v = hfa_view(hfa->words.data());
  P.tables = d_tables;
  P.off = reinterpret_cast<const uint64_t*>(ws->d_desc.p + o_off);
  P.header = ws->d_desc.p + o_hdr;
  P.keep = ws->d_desc.p + o_keep;
  P.nrec = nrec;
  P.flags = flags;
  if ((e = hipEventRecord(ws->tm[0], st)) != hipSuccess) return hip_fail(e, "index query");
  if (flags & UGPU_QUERY_FORCE_LDS) {
    P.stage = kQStageAll;
    hipLaunchKernelGGL((index_query_kernel<kQWavesAll, kQStageAll>), dim3((nrec + kQWavesAll - 1) / kQWavesAll),
                       dim3(kQWavesAll * 64), 0, st, P);
  } else {
    P.stage = (flags & UGPU_QUERY_FORCE_GLOBAL) ? 0 : default_stage();
    hipLaunchKernelGGL((index_query_kernel<kQWaves, kQStage>), dim3((nrec + kQWaves - 1) / kQWaves), dim3(kQWaves * 64), 0,
                       st, P);
  }
  if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(ws->tm[1], st)) != hipSuccess)
    return hip_fail(e, "index query");
  if ((e = hipMemcpyAsync(ws->h_desc.p + o_keep, P.keep, nrec, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "index query result copy");
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ws->tm[0], ws->tm[1]) == hipSuccess) g_query_kernel_ms += ms;
  std::memcpy(keep, ws->h_desc.p + o_keep, nrec);
  return UGPU_OK;
}

struct StoreRec {  // a span of host bytes: one record's table, or the compact tables of a sub-batch
  const uint8_t* table;
  uint64_t size;
};

// the spans of recs[i0, i1) (`total` bytes) back to back into ws->d_tab,
// in pieces through the two halves of the pinned stage
int upload_tables(QueryWs* ws, const std::vector<StoreRec>& recs, uint32_t i0, uint32_t i1, uint64_t total)
{
  hipError_t e = ws->d_tab.reserve(total, total + total / 8, 32);
  if (e == hipSuccess) e = ws->h_stage.reserve(2 * kStagePiece, 2 * kStagePiece);
  if (e != hipSuccess) return hip_fail(e, "index query table buffers");
  uint32_t i = i0;
  uint64_t in_off = 0;
  uint32_t piece = 0;
  for (uint64_t done = 0; done < total; ++piece) {
    const uint64_t m = std::min(kStagePiece, total - done);
    uint8_t* h = ws->h_stage.p + (piece & 1u) * kStagePiece;
    if (piece >= 2 && (e = hipEventSynchronize(ws->ev[piece & 1u])) != hipSuccess) return hip_fail(e, "index query tables");
    for (uint64_t f = 0; f < m;) {
      while (i < i1 && in_off == recs[i].size) ++i, in_off = 0;
      if (i >= i1) return fail(UGPU_DEVICE, "index query tables: sizes do not add up");
      const uint64_t c = std::min<uint64_t>(m - f, recs[i].size - in_off);
      std::memcpy(h + f, recs[i].table + in_off, c);
      f += c;
      in_off += c;
    }
    if ((e = hipMemcpyAsync(ws->d_tab.p + done, h, m, hipMemcpyHostToDevice, ws->st)) != hipSuccess ||
        (e = hipEventRecord(ws->ev[piece & 1u], ws->st)) != hipSuccess)
      return hip_fail(e, "index query tables copy");
    done += m;
  }
  return UGPU_OK;
}

// what every entry point checks first; resets the thread's kernel time
int query_begin(uint32_t flags)
{
  if (flags & ~kQueryFlags) return fail(UGPU_INVAL, "unknown flag");
  if ((flags & UGPU_QUERY_FORCE_LDS) && (flags & UGPU_QUERY_FORCE_GLOBAL)) return fail(UGPU_INVAL, "two ways forced");
  g_query_kernel_ms = 0.f;
  return UGPU_OK;
}

// no automaton: the index skips nothing, every record is kept
bool keep_all(const ugpu_hfa* hfa, uint8_t* keep, uint32_t nrec)
{
  if (!hfa->words.empty()) return false;
  if (nrec) std::memset(keep, 1, nrec);
  return true;
}

}  // namespace

}  // namespace ugpu

// ---------------------------------------------------------------- C ABI
using namespace ugpu;

extern "C" {

uint32_t ugpu_index_query_lds(void) { return default_stage(); }

int ugpu_index_query(const ugpu_hfa* hfa, const uint8_t* d_tables, const uint8_t* header, const uint64_t* offset,
                     uint32_t nrec, uint32_t flags, uint8_t* keep, void* stream)
{
  if (!hfa || (nrec && (!header || !offset || !keep))) return fail(UGPU_INVAL, "NULL argument");
  if (const int bad = query_begin(flags)) return bad;
  if (!nrec || keep_all(hfa, keep, nrec)) return UGPU_OK;
  if (reinterpret_cast<uintptr_t>(d_tables) & 15u) return fail(UGPU_INVAL, "tables must be 16-byte aligned");
  const int rc = check_records(header, offset, nrec);
  if (rc) return rc;
  if (offset[nrec] && !d_tables) return fail(UGPU_INVAL, "NULL tables");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  WsLease<QueryWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "index query workspace");
  return query_records(ws.ws, hfa, d_tables, header, offset, nrec, flags, keep, reinterpret_cast<hipStream_t>(stream));
}

int ugpu_index_query_kernel_ms(float* ms)
{
  if (!ms) return fail(UGPU_INVAL, "NULL argument");
  *ms = g_query_kernel_ms;
  return UGPU_OK;
}

int ugpu_index_query_records(const ugpu_hfa* hfa, const uint8_t* tables, const uint8_t* header, const uint64_t* offset,
                             uint32_t nrec, uint32_t flags, uint8_t* keep)
{
  if (!hfa || (nrec && (!header || !offset || !keep))) return fail(UGPU_INVAL, "NULL argument");
  if (const int bad = query_begin(flags)) return bad;
  if (!nrec || keep_all(hfa, keep, nrec)) return UGPU_OK;
  int rc = check_records(header, offset, nrec);
  if (rc) return rc;
  if (offset[nrec] && !tables) return fail(UGPU_INVAL, "NULL tables");
  for (uint32_t s = 0; s < nrec; ++s)
    if (offset[s] > offset[s + 1]) return fail(UGPU_INVAL, "offsets must ascend");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  WsLease<QueryWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "index query workspace");
  const uint64_t limit = std::max<uint64_t>(q_env("UGPU_BATCH_BYTES", 1ull << 30), 1);
  std::vector<uint64_t> off;
  for (uint32_t i = 0; i < nrec && !rc;) {
    // the next sub-batch: cut only between records
    uint32_t j = i + 1;
    while (j < nrec && offset[j + 1] - offset[i] <= limit) ++j;
    const uint64_t total = offset[j] - offset[i];
    off.resize((size_t)(j - i) + 1);
    for (uint32_t k = i; k <= j; ++k) off[k - i] = offset[k] - offset[i];
    if (total) {  // (compact tables: the sub-batch is one span)
      const std::vector<StoreRec> span{StoreRec{tables + offset[i], total}};
      rc = upload_tables(ws.ws, span, 0, 1, total);
    }
    if (!rc) rc = query_records(ws.ws, hfa, ws->d_tab, header + i, off.data(), j - i, flags, keep + i, ws->st);
    i = j;
  }
  (void)hipStreamSynchronize(ws->st);
  return rc;
}

int ugpu_query_free(ugpu_query_result* r)
{
  if (!r) return UGPU_OK;
  std::free(r->keep);
  std::free(r->header);
  std::free(r->name_blob);
  std::free(r->name_off);
  std::free(r->name_len);
  std::free(r);
  return UGPU_OK;
}

int ugpu_index_query_store(const ugpu_hfa* hfa, const uint8_t* const* blobs, const uint64_t* lens, uint32_t nblobs,
                           uint32_t flags, ugpu_query_result** out)
{
  if (!hfa || !out || (nblobs && (!blobs || !lens))) return fail(UGPU_INVAL, "NULL argument");
  *out = nullptr;
  if (const int bad = query_begin(flags)) return bad;
  // the records (src/ugrep-indexer.cpp:1725-1745)
  std::vector<StoreRec> recs;
  std::vector<uint8_t> header;
  std::vector<uint32_t> nblob, nlen;
  std::vector<uint64_t> noff;
  for (uint32_t bi = 0; bi < nblobs; ++bi) {
    const uint8_t* b = blobs[bi];
    const uint64_t n = lens[bi];
    if (!b || n < 5 || std::memcmp(b, kMagic, 5) != 0) return fail(UGPU_INVAL, "not an index store");
    for (uint64_t p = 5; p < n;) {
      if (n - p < 4) return fail(UGPU_INVAL, "index store: a record is cut");
      const uint32_t h = b[p + 1], lg = h & 0x1Fu, ln = b[p + 2] | (uint32_t)b[p + 3] << 8;
      if (lg && (lg < 7 || lg > 16)) return fail(UGPU_INVAL, "index store: a table has 128 to 65536 bytes");
      const uint64_t size = lg ? 1ull << lg : 0;
      if (n - p - 4 < ln + size) return fail(UGPU_INVAL, "index store: a record is cut");
      if (recs.size() >= 0xFFFFFFFFull) return fail(UGPU_INVAL, "too many records");
      header.push_back((uint8_t)h);
      nblob.push_back(bi), noff.push_back(p + 4), nlen.push_back(ln);
      recs.push_back(StoreRec{b + p + 4 + ln, size});
      p += 4 + ln + size;
    }
  }
  const uint32_t nrec = (uint32_t)recs.size();
  ugpu_query_result* r = static_cast<ugpu_query_result*>(std::calloc(1, sizeof(ugpu_query_result)));
  if (!r) return fail(UGPU_NOMEM, "host allocation");
  r->nrec = nrec;
  r->keep = static_cast<uint8_t*>(std::calloc((uint64_t)nrec + 1, 1));
  r->header = static_cast<uint8_t*>(std::calloc((uint64_t)nrec + 1, 1));
  r->name_blob = static_cast<uint32_t*>(std::calloc((uint64_t)nrec + 1, 4));
  r->name_off = static_cast<uint64_t*>(std::calloc((uint64_t)nrec + 1, 8));
  r->name_len = static_cast<uint32_t*>(std::calloc((uint64_t)nrec + 1, 4));
  if (!r->keep || !r->header || !r->name_blob || !r->name_off || !r->name_len) {
    ugpu_query_free(r);
    return fail(UGPU_NOMEM, "host allocation");
  }
  if (nrec) {
    std::memcpy(r->header, header.data(), nrec);
    std::memcpy(r->name_blob, nblob.data(), 4ull * nrec);
    std::memcpy(r->name_off, noff.data(), 8ull * nrec);
    std::memcpy(r->name_len, nlen.data(), 4ull * nrec);
  }
  if (keep_all(hfa, r->keep, nrec)) {
    *out = r;
    return UGPU_OK;
  }
  const uint64_t limit = std::max<uint64_t>(q_env("UGPU_BATCH_BYTES", 1ull << 30), 1);
  QueryWs* ws = nullptr;
  int rc = UGPU_OK;
  std::vector<uint64_t> off;
  for (uint32_t i = 0; i < nrec && !rc;) {
    // the next sub-batch: cut only between records
    uint32_t j = i;
    uint64_t total = 0;
    for (; j < nrec; ++j) {
      if (j > i && total + recs[j].size > limit) break;
      total += recs[j].size;
    }
    if (!ws) {
      int dev = 0;
      const hipError_t e = hipGetDevice(&dev);
      if (e != hipSuccess) rc = hip_fail(e, "hipGetDevice");
      if (!rc && !(ws = WsLease<QueryWs>::take(dev))) rc = fail(UGPU_NOMEM, "index query workspace");
      if (rc) break;
    }
    off.resize((size_t)(j - i) + 1);
    off[0] = 0;
    for (uint32_t k = i; k < j; ++k) off[k - i + 1] = off[k - i] + recs[k].size;
    if (total) rc = upload_tables(ws, recs, i, j, total);
    if (!rc) rc = query_records(ws, hfa, ws->d_tab, r->header + i, off.data(), j - i, flags, r->keep + i, ws->st);
    i = j;
  }
  if (ws) {
    (void)hipStreamSynchronize(ws->st);
    WsLease<QueryWs>::give(ws);
  }
  if (rc) {
    ugpu_query_free(r);
    return rc;
  }
  *out = r;
  return UGPU_OK;
}

}  // extern "C"
