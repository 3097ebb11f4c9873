// hfa.cpp -- the hash finite automaton of a pattern and its query over an
// index table (host half, libugpu_host.so): what Pattern::gen_match_hfa and
// Pattern::match_hfa do (lib/pattern.cpp:4641-4815), restated over the subset
// DFA of regex_compile.cpp and flattened into arrays (hfa.hpp).
//
// The automaton.  The DFA states reachable in level + 1 bytes from the start,
// level 0..15; per state and level one set of 16-bit hashes per offset,
// offset = max(0, level - 7) .. level: the hashes h' = (61 h + b) mod 2^16 of
// every byte chain that begins at depth `offset` and ends with the state's
// incoming byte.  A state is cut (it gets no successors: "dead", which means
// accept) when it accepts, has no edges, or the target of its lowest edge
// accepts or has no edges (gen_match_hfa_transitions looks at that one edge).
//
// The query walks the levels breadth first with two visit sets that alternate
// and are never cleared; ugpu_hfa_match_host below states every rule.
//
// Truncation.  The reference gives up in the order of its states' addresses;
// here, when the 1024 state ids or kMaxRanges ranges run out, generation stops
// and every entry of the last level is dead, which keeps more files, never
// fewer.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <map>
#include <memory>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "hfa.hpp"
#include "plan.hpp"
#include "subset_dfa.hpp"

namespace ugpu {
namespace {

constexpr uint32_t kHashes = 65536;
constexpr uint64_t kMaxRanges = 1ull << 22;  // 16 MiB of ranges: beyond it the automaton is cut

typedef std::array<uint64_t, kHashes / 64> Bits;

inline void set_bit(Bits& b, uint32_t h) { b[h >> 6] |= 1ull << (h & 63); }

// bits [lo, hi] of b, lo <= hi < 65536
void set_span(Bits& b, uint32_t lo, uint32_t hi)
{
  const uint32_t wl = lo >> 6, wh = hi >> 6;
  const uint64_t ml = ~0ull << (lo & 63), mh = ~0ull >> (63 - (hi & 63));
  if (wl == wh) {
    b[wl] |= ml & mh;
    return;
  }
  b[wl] |= ml;
  for (uint32_t w = wl + 1; w < wh; ++w) b[w] = ~0ull;
  b[wh] |= mh;
}

uint32_t count_bits(const Bits& b)
{
  uint32_t n = 0;
  for (uint64_t w : b) n += (uint32_t)__builtin_popcountll(w);
  return n;
}

// dst |= src rotated up by k places in the ring of 65536 hashes
void or_rotated(Bits& dst, const Bits& src, uint32_t k)
{
  const uint32_t ws = (k >> 6) & 1023u, bs = k & 63u;
  for (uint32_t j = 0; j < 1024; ++j) {
    const uint64_t a = src[(j - ws) & 1023u];
    dst[j] |= bs ? (a << bs) | (src[(j - ws - 1) & 1023u] >> (64 - bs)) : a;
  }
}

// dst |= { (61 h + b) mod 2^16 : h in src, lo <= b <= hi }
void extend(Bits& dst, const Bits& src, uint32_t lo, uint32_t hi)
{
  const uint32_t n = count_bits(src), w = hi - lo + 1;
  if (!n) return;
  if (n == kHashes) {
    dst.fill(~0ull);
    return;
  }
  const bool direct = (uint64_t)n * w <= 4096;
  std::unique_ptr<Bits> t(new Bits);
  t->fill(0);
  for (uint32_t j = 0; j < 1024; ++j)
    for (uint64_t m = src[j]; m; m &= m - 1) {
      const uint32_t h = (61u * (j * 64u + (uint32_t)__builtin_ctzll(m)) + lo) & 0xFFFFu;
      if (!direct)
        set_bit(*t, h);
      else if (h + w - 1 < kHashes)
        set_span(dst, h, h + w - 1);
      else {
        set_span(dst, h, kHashes - 1);
        set_span(dst, 0, (h + w - 1) & 0xFFFFu);
      }
    }
  if (direct) return;
  // the union of w rotations of t, by doubling
  uint32_t cover = 1;
  while (cover * 2 <= w) {
    Bits prev = *t;
    or_rotated(*t, prev, cover);
    cover *= 2;
  }
  if (cover < w) {
    Bits prev = *t;
    or_rotated(*t, prev, w - cover);
  }
  for (uint32_t j = 0; j < 1024; ++j) dst[j] |= (*t)[j];
}

typedef std::array<std::unique_ptr<Bits>, kHfaChain> Sets;  // by offset - first offset of the level
typedef std::map<uint32_t, Sets> Level;                     // by DFA state

inline uint32_t first_offset(uint32_t level) { return level < kHfaChain ? 0 : level + 1 - kHfaChain; }

Bits& set_of(Level& lv, uint32_t state, uint32_t k)
{
  std::unique_ptr<Bits>& p = lv[state][k];
  if (!p) {
    p.reset(new Bits);
    p->fill(0);
  }
  return *p;
}

struct Builder {
  const SubsetDfa& d;
  std::vector<uint32_t> id;                // DFA state -> HFA state id, 0 = none yet
  std::vector<std::set<uint32_t>> succ;    // by HFA id
  uint32_t next_id = 1;
  bool truncated = false;
  // flattened so far
  std::vector<uint32_t> level_first, entry_state, entry_pair, pair_range, range;
  std::vector<uint32_t> entry_level;
  uint64_t hashes = 0;

  explicit Builder(const SubsetDfa& dfa) : d(dfa), id(dfa.next.size(), 0), succ(kHfaStates) {}

  bool has_edges(uint32_t s) const
  {
    for (uint32_t t : d.next[s])
      if (t) return true;
    return false;
  }
  bool final_state(uint32_t s) const { return d.accepting[s] || !has_edges(s); }
  // the state is cut: no successors
  bool cut(uint32_t s) const
  {
    if (final_state(s)) return true;
    for (uint32_t t : d.next[s])
      if (t) return final_state(t);  // (the lowest edge alone decides)
    return true;
  }

  // the edges of s into `to`; false when the state ids ran out (s is then dead)
  bool expand(uint32_t level, uint32_t s, const Sets* prev, Level& to)
  {
    const uint32_t off0 = first_offset(level), poff0 = level ? first_offset(level - 1) : 0;
    for (uint32_t lo = 0; lo < 256;) {
      const uint32_t t = d.next[s][lo];
      uint32_t hi = lo;
      while (hi + 1 < 256 && d.next[s][hi + 1] == t) ++hi;
      if (t) {
        if (!id[t]) {
          if (next_id >= kHfaStates) {
            succ[id[s]].clear();
            truncated = true;
            return false;
          }
          id[t] = next_id++;
        }
        succ[id[s]].insert(id[t]);
        for (uint32_t off = off0; off < level; ++off)
          if ((*prev)[off - poff0]) extend(set_of(to, t, off - off0), *(*prev)[off - poff0], lo, hi);
        set_span(set_of(to, t, level - off0), lo, hi);
      }
      lo = hi + 1;
    }
    return true;
  }

  void flatten(uint32_t level, const Level& lv)
  {
    std::map<uint32_t, const Sets*> by_id;  // (the reference keeps a level's entries by state id)
    for (const auto& kv : lv) by_id[id[kv.first]] = &kv.second;
    const uint32_t npair = std::min(level, kHfaChain - 1) + 1;
    for (const auto& kv : by_id) {
      entry_state.push_back(kv.first);
      entry_level.push_back(level);
      entry_pair.push_back((uint32_t)pair_range.size());
      for (uint32_t k = 0; k < npair; ++k) {
        pair_range.push_back((uint32_t)range.size());
        const Bits* b = (*kv.second)[k].get();
        if (!b) continue;
        hashes += count_bits(*b);
        for (uint32_t h = 0; h < kHashes;) {
          const uint64_t w = (*b)[h >> 6] >> (h & 63);
          if (!w) {
            h = (h | 63u) + 1;
            continue;
          }
          h += (uint32_t)__builtin_ctzll(w);
          uint32_t e = h;  // the run [h, e]
          while (e + 1 < kHashes) {
            const uint64_t x = ~((*b)[(e + 1) >> 6] >> ((e + 1) & 63));  // zeros behind the run
            const uint32_t room = 64 - ((e + 1) & 63);
            const uint32_t ones = x ? (uint32_t)__builtin_ctzll(x) : 64;
            if (ones < room) {
              e += ones;
              break;
            }
            e += room;
          }
          range.push_back(h | (e << 16));
          h = e + 1;
        }
      }
    }
  }

  // the words (hfa.hpp); empty when the pattern has no automaton
  std::vector<uint32_t> build(ugpu_hfa_info_t& info)
  {
    std::vector<uint32_t> words;
    const uint32_t start = 1;
    if (d.next.size() < 2 || final_state(start)) return words;
    id[start] = next_id++;
    Level cur;
    expand(0, start, nullptr, cur);
    uint32_t levels = 0;
    for (uint32_t level = 0; level < kHfaDepth && !cur.empty(); ++level) {
      level_first.push_back((uint32_t)entry_state.size());
      flatten(level, cur);
      levels = level + 1;
      if (range.size() > kMaxRanges) truncated = true;
      if (truncated || level + 1 == kHfaDepth) break;
      Level nxt;
      for (const auto& kv : cur)
        if (!cut(kv.first) && !expand(level + 1, kv.first, &kv.second, nxt)) break;
      cur.swap(nxt);
    }
    const uint32_t E = (uint32_t)entry_state.size();
    while (level_first.size() < kHfaDepth + 1) level_first.push_back(E);
    entry_pair.push_back((uint32_t)pair_range.size());
    pair_range.push_back((uint32_t)range.size());
    std::vector<uint32_t> entry_dead(E), entry_succ, succs;
    for (uint32_t e = 0; e < E; ++e) {
      const std::set<uint32_t>& s = succ[entry_state[e]];
      // (a cut automaton's last level is dead whatever its states led to earlier)
      entry_dead[e] = s.empty() || (truncated && entry_level[e] + 1 == levels);
      entry_succ.push_back((uint32_t)succs.size());
      if (!entry_dead[e]) succs.insert(succs.end(), s.begin(), s.end());
    }
    entry_succ.push_back((uint32_t)succs.size());
    words = {kHfaMagic, levels, E, (uint32_t)pair_range.size() - 1, (uint32_t)range.size(), (uint32_t)succs.size(),
             next_id, truncated ? 1u : 0u};
    for (const std::vector<uint32_t>* a : {&level_first, &entry_state, &entry_dead, &entry_pair, &entry_succ, &pair_range,
                                           &succs, &range})
      words.insert(words.end(), a->begin(), a->end());
    info.has_hfa = 1, info.levels = levels, info.states = next_id - 1, info.entries = E;
    info.ranges = (uint32_t)range.size(), info.hashes = hashes, info.truncated = truncated;
    return words;
  }
};

// whether `n` words are a well-formed automaton: every index the evaluators
// follow stays inside its array
bool valid_words(const uint32_t* w, uint64_t n, std::string& why)
{
  if (n < kHfaHead + kHfaDepth + 1 || w[0] != kHfaMagic) return why = "not an HFA", false;
  if (w[1] > kHfaDepth || w[6] > kHfaStates) return why = "too many levels or states", false;
  for (int i = 2; i <= 5; ++i)
    if (w[i] > (1u << 28)) return why = "count too large", false;
  const HfaView v = hfa_view(w);
  if (v.end != n) return why = "length does not match the counts", false;
  auto csr = [&](uint32_t at, uint32_t cnt, uint32_t total) {
    if (w[at] != 0 || w[at + cnt] != total) return false;
    for (uint32_t i = 0; i < cnt; ++i)
      if (w[at + i] > w[at + i + 1]) return false;
    return true;
  };
  if (!csr(v.entry_pair, v.entries, v.pairs) || !csr(v.entry_succ, v.entries, v.succs) ||
      !csr(v.pair_range, v.pairs, v.ranges))
    return why = "offsets do not ascend", false;
  if (w[v.level_first] != 0 || w[v.level_first + kHfaDepth] != v.entries) return why = "level bounds", false;
  for (uint32_t l = 0; l < kHfaDepth; ++l) {
    const uint32_t a = w[v.level_first + l], b = w[v.level_first + l + 1];
    if (a > b || b > v.entries || (l >= v.levels && a != b)) return why = "level bounds", false;
    for (uint32_t e = a; e < b; ++e)
      if (w[v.entry_pair + e + 1] - w[v.entry_pair + e] != std::min(l, kHfaChain - 1) + 1)
        return why = "an entry's offsets do not fit its level", false;
  }
  for (uint32_t e = 0; e < v.entries; ++e)
    if (w[v.entry_state + e] >= v.states || w[v.entry_dead + e] > 1) return why = "entry state", false;
  for (uint32_t i = 0; i < v.succs; ++i)
    if (w[v.succ + i] >= v.states) return why = "successor state", false;
  for (uint32_t i = 0; i < v.ranges; ++i)
    if ((w[v.range + i] & 0xFFFFu) > (w[v.range + i] >> 16)) return why = "range", false;
  return true;
}

void info_of_words(const std::vector<uint32_t>& w, ugpu_hfa_info_t& info)
{
  memset(&info, 0, sizeof(info));
  if (w.empty()) return;
  const HfaView v = hfa_view(w.data());
  info.has_hfa = v.levels != 0, info.levels = v.levels, info.entries = v.entries, info.ranges = v.ranges;
  info.truncated = w[7] & 1u;
  std::set<uint32_t> st;
  for (uint32_t e = 0; e < v.entries; ++e) st.insert(w[v.entry_state + e]);
  info.states = (uint32_t)st.size();
  for (uint32_t i = 0; i < v.ranges; ++i) info.hashes += (w[v.range + i] >> 16) - (w[v.range + i] & 0xFFFFu) + 1;
}

// Pattern::match_hfa over one table of `size` bytes (a power of two): keep?
bool match_words(const std::vector<uint32_t>& words, const uint8_t* table, uint32_t size)
{
  const uint32_t* w = words.data();
  const HfaView v = hfa_view(w);
  const uint32_t mask = size - 1;
  uint8_t visit[2][kHfaStates];  // alternate by level & 1 and are never cleared
  memset(visit, 0, sizeof(visit));
  for (uint32_t level = 0; level < kHfaDepth; ++level) {
    const uint8_t* cur = visit[level & 1];
    uint8_t* nxt = visit[~level & 1];
    bool any = false;
    for (uint32_t e = w[v.level_first + level]; e < w[v.level_first + level + 1]; ++e) {
      if (level && !cur[w[v.entry_state + e]]) continue;  // (level 0 tests every entry)
      bool all = true;
      const uint32_t p0 = w[v.entry_pair + e], p1 = w[v.entry_pair + e + 1];
      for (uint32_t p = p0; p < p1; ++p) {
        const uint8_t bit = (uint8_t)(1u << (p1 - 1 - p));  // 1 << (level - offset)
        bool flag = false;
        for (uint32_t r = w[v.pair_range + p]; r < w[v.pair_range + p + 1] && !flag; ++r) {
          const uint32_t lo = w[v.range + r] & 0xFFFFu, hi = w[v.range + r] >> 16;
          const uint32_t n = std::min<uint32_t>(hi - lo + 1, size);  // a longer range meets every slot
          for (uint32_t i = 0; i < n && !flag; ++i) flag = !(table[(lo + i) & mask] & bit);
        }
        if (!flag) {
          all = false;
          break;
        }
        // the successors are marked once an offset passes, the first included,
        // whatever the later offsets say; a dead state ends the query at once
        if (w[v.entry_dead + e]) return true;
        for (uint32_t s = w[v.entry_succ + e]; s < w[v.entry_succ + e + 1]; ++s) nxt[w[v.succ + s]] = 1;
      }
      any = any || all;
    }
    if (!any) return false;
  }
  return true;
}

std::atomic<uint64_t> g_hfa_id{1};

}  // namespace
}  // namespace ugpu

using namespace ugpu;

extern "C" {

int ugpu_hfa_create(const char* regex, size_t len, uint32_t flags, ugpu_hfa** out)
{
  if (!out || (!regex && len)) return host_fail(UGPU_INVAL, "NULL argument");
  *out = nullptr;
  if (flags & ~(UGPU_RX_FIXED | UGPU_RX_ICASE | UGPU_RX_REFLEX)) return host_fail(UGPU_INVAL, "unknown flag");
  try {
    SubsetDfa d;
    const int rc = subset_dfa(regex, len, flags, d);
    if (rc) return host_fail(rc, ugpu_compile_error());
    std::unique_ptr<ugpu_hfa> h(new ugpu_hfa);
    h->id = g_hfa_id.fetch_add(1);
    memset(&h->info, 0, sizeof(h->info));
    Builder b(d);
    h->words = b.build(h->info);
    *out = h.release();
    return UGPU_OK;
  } catch (const std::bad_alloc&) {
    return host_fail(UGPU_NOMEM, "host allocation");
  }
}

int ugpu_hfa_import(const uint32_t* words, uint64_t nwords, ugpu_hfa** out)
{
  if (!out || !words) return host_fail(UGPU_INVAL, "NULL argument");
  *out = nullptr;
  std::string why;
  if (!valid_words(words, nwords, why)) return host_fail(UGPU_INVAL, "HFA words: " + why);
  try {
    std::unique_ptr<ugpu_hfa> h(new ugpu_hfa);
    h->id = g_hfa_id.fetch_add(1);
    if (words[1]) h->words.assign(words, words + nwords);
    info_of_words(h->words, h->info);
    *out = h.release();
    return UGPU_OK;
  } catch (const std::bad_alloc&) {
    return host_fail(UGPU_NOMEM, "host allocation");
  }
}

int ugpu_hfa_export(const ugpu_hfa* hfa, uint32_t* words, uint64_t capacity, uint64_t* nwords)
{
  if (!hfa || !nwords) return host_fail(UGPU_INVAL, "NULL argument");
  *nwords = hfa->words.size();
  if (!words) return UGPU_OK;
  if (capacity < hfa->words.size()) return host_fail(UGPU_CAPACITY, "HFA words do not fit");
  if (!hfa->words.empty()) memcpy(words, hfa->words.data(), hfa->words.size() * sizeof(uint32_t));
  return UGPU_OK;
}

int ugpu_hfa_destroy(ugpu_hfa* hfa)
{
  delete hfa;
  return UGPU_OK;
}

int ugpu_hfa_info(const ugpu_hfa* hfa, ugpu_hfa_info_t* info)
{
  if (!hfa || !info) return host_fail(UGPU_INVAL, "NULL argument");
  *info = hfa->info;
  return UGPU_OK;
}

int ugpu_hfa_match_host(const ugpu_hfa* hfa, const uint8_t* table, uint64_t size, int* keep)
{
  if (!hfa || !keep || !table) return host_fail(UGPU_INVAL, "NULL argument");
  if (size < 1 || size > kHashes || (size & (size - 1))) return host_fail(UGPU_INVAL, "table size is a power of two up to 65536");
  *keep = hfa->words.empty() || match_words(hfa->words, table, (uint32_t)size);  // no automaton: nothing can be skipped
  return UGPU_OK;
}

int ugpu_hfa_query_host(const ugpu_hfa* hfa, const uint8_t* tables, const uint8_t* header, const uint64_t* offset,
                        uint32_t nrec, uint32_t flags, uint8_t* keep)
{
  if (!hfa || (nrec && (!header || !offset || !keep))) return host_fail(UGPU_INVAL, "NULL argument");
  if (flags & ~(UGPU_QUERY_IGNORE_BINARY | UGPU_QUERY_DECOMPRESS | UGPU_QUERY_FORCE_LDS | UGPU_QUERY_FORCE_GLOBAL))
    return host_fail(UGPU_INVAL, "unknown flag");
  if (hfa->words.empty()) {  // no automaton: the index skips nothing
    if (nrec) memset(keep, 1, nrec);
    return UGPU_OK;
  }
  for (uint32_t s = 0; s < nrec; ++s) {
    const uint32_t b = header[s], lg = b & 0x1Fu;
    if (lg > 16) return host_fail(UGPU_INVAL, "a table has up to 65536 bytes");
    if (lg && (!tables || offset[s] > offset[nrec] || (1ull << lg) > offset[nrec] - offset[s]))
      return host_fail(UGPU_INVAL, "a table lies outside the tables");
  }
  for (uint32_t s = 0; s < nrec; ++s) {
    const uint32_t b = header[s], lg = b & 0x1Fu;
    if (((b & 0x80u) && (flags & UGPU_QUERY_IGNORE_BINARY)) || ((b & 0x60u) && !(flags & UGPU_QUERY_DECOMPRESS)))
      keep[s] = 0;
    else if (!lg)
      keep[s] = (b & 0x80u) ? 1 : 0;
    else
      keep[s] = match_words(hfa->words, tables + offset[s], 1u << lg);
  }
  return UGPU_OK;
}

}  // extern "C"
