// hfa_asan.cpp -- the host half of the index query (hfa.cpp: ugpu_hfa_create,
// export / import, ugpu_hfa_match_host) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program linked to the instrumented
// host sources (tools/asan/Makefile, `make -C tools/asan hfa`).  It builds the
// automata of the patterns of tests/golden/hfa_cases.json (restated here; the
// set of 100 words is a seeded set of its own, of the same shape) and
// evaluates each over tables of 128 to 65536 bytes hashed from a few texts,
// the original and its re-imported export, which must agree.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "ugpu.h"

namespace {

// the indexer's table of `text`, folded by halving down to `size` bytes
std::vector<uint8_t> table_of(const std::string& text, size_t size)
{
  std::vector<uint8_t> t(65536, 0xFF);
  for (size_t i = 0; i < text.size(); ++i) {
    uint32_t h = (uint8_t)text[i];
    t[h] &= 0xFE;
    for (size_t k = 1; k < 8 && i + k < text.size(); ++k) {
      h = (61 * h + (uint8_t)text[i + k]) & 0xFFFF;
      t[h] &= (uint8_t)~(1u << k);
    }
  }
  for (size_t n = 65536; n > size; n /= 2)
    for (size_t i = 0; i < n / 2; ++i) t[i] &= t[i + n / 2];
  t.resize(size);
  return t;
}

struct Pat {
  const char* rx;
  uint32_t flags;
};

}  // namespace

int main()
{
  const char lit26[] = "abcdefghijklmnopqrstuvwxyz";
  std::string words = "kernel|bloom";
  uint32_t seed = 7;
  for (int i = 0; i < 98; ++i) {
    words += "|";
    for (int k = 0; k < 4 + i % 5; ++k) {
      seed = seed * 1103515245u + 12345u;
      words += (char)('a' + (seed >> 16) % 26);
    }
  }
  const std::vector<Pat> pats = {
      {"a", 0}, {"of", 0}, {"the that", 0}, {"with be b", 0}, {"record store bin", 0}, {"record store bina", 0},
      {lit26, 0}, {"kernel", 0}, {"zyzzyva", 0}, {"needle07", 0}, {"needle0[1-3]", 0}, {"needle(07|19)x?", 0},
      {"hash|bloom", 0}, {"the|thereof", 0}, {"ab|abcd", 0}, {"a(bc)*d", 0}, {"n(ee)+dle", 0}, {"[a-z]+que", 0},
      {"[a-z]{3}ord", 0}, {"recor[a-z]", 0}, {"tab.e", 0}, {"zq[0-9]+x", 0}, {"[0-9]{4}", 0}, {"\\w+", 0},
      {"[^a-z ]{2}", 0}, {"\xc3\xa9+", 0}, {"\xce\xb1|\xe2\x82\xac", 0}, {"[\\x80-\\xff]e", 0}, {"a*", 0},
      {"kernel\\b", 0}, {"^index", 0}, {words.c_str(), 0}, {"kernel", UGPU_RX_ICASE}, {"a(bc)*d", UGPU_RX_FIXED},
      {"a+?b", 0}, {"(", 0}};
  std::string text = "the kernel of the index table hash file bloom gram noise fold record store binary antique\n";
  std::string big;
  for (int i = 0; i < 400; ++i) big += text + std::to_string(i * 2654435761u) + " needle19x abcbcd zq7x 2024\n";
  const std::vector<std::vector<uint8_t>> tables = {table_of("", 128), table_of(text, 128), table_of(text, 256),
                                                    table_of(big, 4096), table_of(big, 65536)};
  int built = 0, refused = 0, kept = 0, asked = 0;
  for (const Pat& p : pats) {
    ugpu_hfa* h = nullptr;
    const int rc = ugpu_hfa_create(p.rx, strlen(p.rx), p.flags, &h);
    if (rc != UGPU_OK) {
      ++refused;
      continue;
    }
    ++built;
    uint64_t n = 0;
    if (ugpu_hfa_export(h, nullptr, 0, &n) != UGPU_OK) return 2;
    std::vector<uint32_t> w(n + 1);
    if (ugpu_hfa_export(h, w.data(), n, &n) != UGPU_OK) return 2;
    ugpu_hfa* h2 = nullptr;
    if (n && ugpu_hfa_import(w.data(), n, &h2) != UGPU_OK) return 3;
    if (n > 8) {  // a cut copy is refused, not followed
      ugpu_hfa* h3 = nullptr;
      if (ugpu_hfa_import(w.data(), n - 1, &h3) == UGPU_OK) return 4;
    }
    for (const std::vector<uint8_t>& t : tables) {
      int a = -1, b = -1;
      if (ugpu_hfa_match_host(h, t.data(), t.size(), &a) != UGPU_OK) return 5;
      if (h2 && (ugpu_hfa_match_host(h2, t.data(), t.size(), &b) != UGPU_OK || a != b)) return 6;
      kept += a;
      ++asked;
    }
    ugpu_hfa_info_t info;
    if (ugpu_hfa_info(h, &info) != UGPU_OK) return 7;
    ugpu_hfa_destroy(h2);
    ugpu_hfa_destroy(h);
  }
  printf("hfa_asan: %d automata built, %d patterns refused, %d of %d tables kept\n", built, refused, kept, asked);
  return built >= 30 && refused == 2 && kept > 0 && kept < asked ? 0 : 1;
}
