// plan.hpp -- the host half of the engine (libugpu_host.so), shared with the
// device half (engine.hip in libugrep_amd.so).
//
// The host half holds everything a caller needs to decide, without a device,
// whether and how a pattern runs on the GPU: the table builder (tables.cpp),
// the regex compiler (regex_compile.cpp), the plan below, the host-only C ABI
// (ugpu_compile, ugpu_dfa_plan_host, ugpu_tables_*_host) and the error string
// of both halves (ugpu_last_error).  It does not link the HIP runtime, so the
// drop-in matcher links only it and loads the device half at the first input
// its policy sends to a GPU (integration/reflex_gpu_matcher.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "tables.hpp"

// Unicode Word ranges as flat [lo, hi] pairs (regex_compile.cpp, the table of \w)
void ugpu_word_ranges(std::vector<uint32_t>& out);

namespace ugpu {

// What ugpu_dfa_create uploads for a table under pattern flags, and so which
// kernels its scans run: decided on the host alone (ugpu_dfa_plan_host answers
// it without touching a device)
constexpr int kLbNeedles = 16;

struct DfaPlan {
  bool ok = true;  // false: option W with line anchors or empty matches (UGPU_UNSUPPORTED)
  bool nul = false, amode = false;
  bool wtab = false, wplus = false, xcw = false;
  bool xtrans = false, xid = false, xu = false, xg = false;
  // loop-needle table (C+ N for a finite set N of strings over C,
  // host_api.cpp loop_needle): the sparse kernel's prefilter looks for the
  // strings of N and its candidates walk back to their C-run's start
  bool lb = false;
  // option W on a byte table without a selective prefilter: the sparse
  // kernel's W walks from the first-byte candidates that follow no ASCII
  // letter (ScanParams::wstart) instead of wfind_kernel (UGPU_WSPARSE)
  bool wsparse = false;
  uint32_t lb_cls[8] = {};
  std::vector<std::string> lb_needles;  // (N, at most kLbNeedles strings of 2-32 bytes)
  uint8_t lb_ft[20] = {};               // the prefilter over N (tables.cpp needle_filter)
  double lb_density = 0;                // its estimated candidate fraction
};

// lb: loop-needle lookback 1 / 0, or -1 for the UGPU_LB default (on)
DfaPlan dfa_plan(const DfaTables& t, uint32_t flags, int lb = -1);
// The two-field prefilter (tables.hpp filter2) on the plain sparse path: a
// first-byte prefilter walked by the plain walk (no loop needle, option W or
// context accepts).  UGPU_FT2=0 / 1, read per call, forces it off / on there.
bool plan_filter2(const DfaTables& t, const DfaPlan& p);
// The n-gram kernel (kernel 7, ngram_kernel.hip; tables.hpp ng_*): a class or
// wide table without context accepts, lookahead, REDO or option N that would
// otherwise scan on dense_kernel (kernel 1) or, for being wide or under option
// W, on wfind_kernel (kernel 4), and whose filter is selective
// (ng_density <= kNgramBound).  UGPU_NG=0, read per call, turns it off.
bool plan_ngram(const DfaTables& t, const DfaPlan& p);

// The scan kernels, numbered as ugpu_dfa_info::kernel reports them
enum Kernel : uint8_t { K_SPARSE = 0, K_DENSE = 1, K_XI = 2, K_XG = 3, K_WFIND = 4, K_XC = 5, K_XU = 6, K_NGRAM = 7 };
constexpr int kKernels = 8;
// xc_kernel's U mode (K_XU) variants: the exact main loop in the fast one's
// place, and the run-edge check of option W on \w+
enum : uint8_t { U_FAST = 0, U_EXACT = 1, U_EDGE = 2 };

// One step of a scan: a kernel over the whole range, then the stitch
struct Step {
  Kernel k = K_DENSE;
  bool w = false;      // the kernel applies the option-W rules (the word table is passed)
  uint8_t u = U_FAST;  // K_XU only
};
inline bool operator==(const Step& a, const Step& b) { return a.k == b.k && a.w == b.w && a.u == b.u; }
inline bool operator!=(const Step& a, const Step& b) { return !(a == b); }

// How option W is served: by every kernel of the route itself (W_EXACT), by
// non-W kernels on valid UTF-8 for tables equivalent to \w+ (W_PLUS, DESIGN
// 3.8), or by xc_kernel on ASCII input (W_XC); the last two redo on `wslow`
enum WMode : uint8_t { W_NONE, W_EXACT, W_PLUS, W_XC };

// The kernels a table's scans run (DESIGN "kernel routes")
struct Route {
  Step count;               // a COUNT scan
  Kernel record = K_DENSE;  // writes its records: count.k, or dense_kernel after xi / xg
  WMode wmode = W_NONE;
  bool ngram = false;       // the n-gram kernel stands in for dense_kernel / wfind_kernel (plan_ngram)
  // where a range is redone when its scan flags
  Step umix;   // UGPU_FLAG_UMIX: U mode's exact kernel
  Step wslow;  // UGPU_FLAG_WSLOW (W_PLUS: or USLOW, or a first step off the fast path): the exact W kernel
  Step uslow;  // UGPU_FLAG_USLOW: the table's kernel behind xc_kernel (xi / xg / dense)
};
// the kernel that writes the records of a COUNT scan on k
constexpr Kernel record_kernel(Kernel k) { return k == K_XI || k == K_XG ? K_DENSE : k; }
// The route of a table under its plan.  Reads the test knobs when it is called:
// UGPU_SPARSE, UGPU_XI, UGPU_XG, UGPU_XC, UGPU_XU, UGPU_XUW, UGPU_NG (= 0: that
// kernel is off).  A scanner still demotes a kernel whose occupancy is 0.
Route dfa_route(const DfaTables& t, const DfaPlan& p);
// r without kernel k (K_XI, K_XG, K_XC or K_XU: its occupancy on the device is
// 0): dense_kernel in xi / xg's place, the kernel behind it in xc_kernel's
inline Route route_demote(Route r, Kernel k)
{
  if (r.uslow.k == k) r.uslow.k = K_DENSE;
  if (r.count.k == k) r.count.k = r.uslow.k, r.count.u = U_FAST;
  r.record = record_kernel(r.count.k);
  r.umix = r.count;
  r.umix.u |= U_EXACT;
  return r;
}
// ugpu_dfa_info from the tables and the plan (ugpu_dfa_plan_host, ugpu_dfa_info_get)
void dfa_info_fill(const DfaTables& t, const DfaPlan& p, void* info /* ugpu_dfa_info* */);
// \w+ as ugpu_compile builds it
bool is_word_plus(const DfaTables& t);
// sets the calling thread's error string (ugpu_last_error) and returns code
int host_fail(int code, const std::string& msg);

}  // namespace ugpu
