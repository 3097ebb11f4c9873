// hfa.hpp -- the flattened hash finite automaton (hfa.cpp builds and evaluates
// it on the host, index_query.hip on the device).
//
// One array of 32-bit words, the form ugpu_hfa_export hands out:
//   [0] kHfaMagic   [1] levels L (0..16; 0: no automaton)   [2] entries E
//   [3] pairs P     [4] ranges R   [5] successors S          [6] states (ids < this, <= 1024)
//   [7] flags (bit 0: truncated)
//   level_first[17]  entries of level l: [level_first[l], level_first[l+1])
//   entry_state[E]   the entry's state id
//   entry_dead[E]    1: the state has no successors (dead = accept)
//   entry_pair[E+1]  the entry's (entry, offset) pairs; an entry of level l has
//                    min(l, 7) + 1 of them, for offset max(0, l - 7) .. l in order,
//                    so pair k tests bit min(l, 7) - k
//   entry_succ[E+1]  the entry's successors in succ[]
//   pair_range[P+1]  the pair's hash ranges in range[]
//   succ[S]          state ids
//   range[R]         lo | hi << 16, inclusive, lo <= hi, sorted and disjoint per pair
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/ugpu.h"

namespace ugpu {

constexpr uint32_t kHfaMagic = 0x31414648u;  // "HFA1"
constexpr uint32_t kHfaDepth = 16;           // HFA::MAX_DEPTH
constexpr uint32_t kHfaChain = 8;            // HFA::MAX_CHAIN
constexpr uint32_t kHfaStates = 1024;        // HFA::MAX_STATES
constexpr uint32_t kHfaHead = 8;

// the arrays' places in the words
struct HfaView {
  uint32_t levels, entries, pairs, ranges, succs, states;
  uint32_t level_first, entry_state, entry_dead, entry_pair, entry_succ, pair_range, succ, range, end;
};

inline HfaView hfa_view(const uint32_t* w)
{
  HfaView v;
  v.levels = w[1], v.entries = w[2], v.pairs = w[3], v.ranges = w[4], v.succs = w[5], v.states = w[6];
  v.level_first = kHfaHead;
  v.entry_state = v.level_first + kHfaDepth + 1;
  v.entry_dead = v.entry_state + v.entries;
  v.entry_pair = v.entry_dead + v.entries;
  v.entry_succ = v.entry_pair + v.entries + 1;
  v.pair_range = v.entry_succ + v.entries + 1;
  v.succ = v.pair_range + v.pairs + 1;
  v.range = v.succ + v.succs;
  v.end = v.range + v.ranges;
  return v;
}

}  // namespace ugpu

struct ugpu_hfa {
  uint64_t id = 0;              // distinct per object: the device half's upload key
  std::vector<uint32_t> words;  // empty: no automaton, every file is kept
  ugpu_hfa_info_t info{};
};
