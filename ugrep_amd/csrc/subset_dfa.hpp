// subset_dfa.hpp -- what hfa.cpp takes from regex_compile.cpp: the subset DFA
// of a pattern before minimisation.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ugpu {

struct SubsetDfa {
  std::vector<std::vector<uint32_t>> next;  // state -> 256 targets; 0 = no edge, 1 = the start state
  std::vector<uint8_t> accepting;           // state accepts (in some context of its assertions)
};

// UGPU_OK, or ugpu_compile's code with the message in ugpu_compile_error()
int subset_dfa(const char* regex, size_t len, uint32_t flags, SubsetDfa& out);

}  // namespace ugpu
