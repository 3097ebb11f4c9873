// columns.hip -- column numbers of byte positions (the
// -k of ugrep -onkb).
//
// Replaces, for a fully buffered input, the per-byte loop of
// AbstractMatcher::columno() (include/reflex/absmatcher.h:795-816) from the
// begin of the line to each match: a '\t' does k += 1 + (~k & (T - 1)), any
// other byte k += ((byte & 0xC0) != 0x80); T is ugrep's --tabs (1, 2, 4, 8).
//
// The fold is not additive over a tab, but a byte range without '\n' is one of
// two functions of the column k at its first byte: k + a when it holds no
// tab, ((k + a) | (T-1)) + 1 + b when it does (a: columns before its first
// tab; b: columns added behind it, which do not depend on k because the column
// behind a tab is a multiple of T).  A range with a '\n' is the constant "its
// tail behind the last newline applied to 0".  These compose associatively
// (compose() below), so the pass is a scan: per 16-byte granule from three
// 16-bit masks (newline, tab, continuation byte), over the four granules of a
// lane (each lane loads 64 consecutive bytes of the tile, so that one wave
// scan per tile is enough), across lanes with DPP, across tiles in registers,
// across wave ranges on the host.
//
// Same wave-range layout as lines.hip (4 KiB tiles, tpw tiles per wave):
//   col_summary_kernel  per wave range: newline count, 1 + position of its
//                       last newline, and its column function;
//   (host)              column_stitch (line_host.hpp): newlines before, line
//                       begin and column at each range's first byte, 64-bit;
//   col_assign_kernel   walks the ascending positions alongside the bytes, 64
//                       per step (as nl_assign_kernel): per tile the granule
//                       masks, the newline prefix, the last newline before and
//                       the scanned column function of every granule go to
//                       LDS; a position takes its granule's entry state and
//                       folds the at most 15 bytes before it from the masks.
#include "device_common.hpp"
#include "line_host.hpp"
#include "line_tiles.hpp"

namespace ugpu {

namespace {

struct ColFn {
  uint32_t kind, a, b;  // kColAdd / kColTab / kColConst (scan_kernels.hpp); all zero: the identity
};

// first f, then g
__device__ __forceinline__ ColFn compose(const ColFn& f, const ColFn& g, uint32_t tm)
{
  const bool ftab = f.kind == kColTab, gtab = g.kind == kColTab;
  const uint32_t x = (ftab ? f.b : f.a) + g.a;  // columns behind f's first tab (f's constant, f's sum) at g's first tab
  const uint32_t y = gtab ? (x | tm) + 1u + g.b : x;
  ColFn r;
  r.kind = f.kind, r.a = ftab ? f.a : y, r.b = ftab ? y : 0u;
  if (f.kind == kColAdd && gtab) r.kind = kColTab, r.a = x, r.b = g.b;
  if (g.kind == kColConst) r = g;
  return r;
}

__device__ __forceinline__ uint64_t apply(const ColFn& f, uint64_t k, uint32_t tm)
{
  if (f.kind == kColConst) return f.a;
  if (f.kind == kColTab) return ((k + f.a) | tm) + 1u + f.b;
  return k + f.a;
}

template <int CTRL, int ROWS>
__device__ __forceinline__ ColFn fn_dpp(const ColFn& v)
{
  ColFn p;  // (lanes without a source get 0: the identity)
  p.kind = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.kind, CTRL, ROWS, 0xf, false);
  p.a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.a, CTRL, ROWS, 0xf, false);
  p.b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.b, CTRL, ROWS, 0xf, false);
  return p;
}

// inclusive wave scan under compose (the steps of lscan_add)
__device__ __forceinline__ ColFn fn_scan(ColFn v, uint32_t tm)
{
  v = compose(fn_dpp<0x111, 0xf>(v), v, tm);
  v = compose(fn_dpp<0x112, 0xf>(v), v, tm);
  v = compose(fn_dpp<0x114, 0xf>(v), v, tm);
  v = compose(fn_dpp<0x118, 0xf>(v), v, tm);
  v = compose(fn_dpp<0x142, 0xa>(v), v, tm);
  v = compose(fn_dpp<0x143, 0xc>(v), v, tm);
  return v;
}

__device__ __forceinline__ ColFn fn_lane63(const ColFn& v)
{
  ColFn r;
  r.kind = (uint32_t)__builtin_amdgcn_readlane((int)v.kind, 63);
  r.a = (uint32_t)__builtin_amdgcn_readlane((int)v.a, 63);
  r.b = (uint32_t)__builtin_amdgcn_readlane((int)v.b, 63);
  return r;
}

// bit 7 of each byte set iff the byte is B (nl_bits for any byte)
template <uint32_t B>
__device__ __forceinline__ uint32_t eq_bits(uint32_t x)
{
  const uint32_t t = x ^ (B * 0x01010101u);
  const uint32_t nz = ((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t;
  return ~nz & 0x80808080u;
}

// bit 7 of each byte set iff it is a UTF-8 continuation byte (10xxxxxx)
__device__ __forceinline__ uint32_t cont_bits(uint32_t x) { return x & ~(x << 1) & 0x80808080u; }

// the bit 7 of every byte of x (to bits 0..3) and of y (to bits 4..7): one
// multiply gathers both, no two partial products meet in a bit
__device__ __forceinline__ uint32_t pack8(uint32_t x, uint32_t y)
{
  return ((((x >> 7) | (y >> 3)) * 0x00204081u) >> 21) & 0xffu;
}

__device__ __forceinline__ uint32_t pack16(uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
  return pack8(x, y) | (pack8(z, w) << 8);
}

struct GMasks {
  uint32_t nl, tab, plain;  // plain: the bytes that count 1 (not a tab, not a continuation byte)
};

__device__ __forceinline__ GMasks granule_masks(const uint4& v, uint32_t valid)
{
  GMasks m;
  m.nl = pack16(nl_bits(v.x), nl_bits(v.y), nl_bits(v.z), nl_bits(v.w)) & valid;
  m.tab = pack16(eq_bits<9>(v.x), eq_bits<9>(v.y), eq_bits<9>(v.z), eq_bits<9>(v.w)) & valid;
  const uint32_t cont = pack16(cont_bits(v.x), cont_bits(v.y), cont_bits(v.z), cont_bits(v.w));
  m.plain = ~cont & ~m.tab & valid;
  return m;
}

__device__ __forceinline__ uint32_t below(uint32_t n) { return (1u << n) - 1u; }  // n <= 16

// the column fold over bytes [s, e) of a granule without a newline in them, from column k
template <class K>
__device__ __forceinline__ K fold(K k, uint32_t tab, uint32_t plain, uint32_t s, uint32_t e, uint32_t tm)
{
  uint32_t m = tab & below(e) & ~below(s);
  while (m) {
    const uint32_t i = (uint32_t)__builtin_ctz(m);
    k += __popc(plain & below(i) & ~below(s));
    k = (k | tm) + 1u;
    s = i + 1u;
    m &= m - 1u;
  }
  return k + __popc(plain & below(e) & ~below(s));
}

__device__ __forceinline__ ColFn granule_fn(const GMasks& m, uint32_t tm)
{
  ColFn f;
  f.b = 0;
  if (m.nl) {
    f.kind = kColConst;
    f.a = fold<uint32_t>(0u, m.tab, m.plain, 32u - (uint32_t)__builtin_clz(m.nl), 16u, tm);
  } else if (m.tab) {
    const uint32_t i = (uint32_t)__builtin_ctz(m.tab);
    f.kind = kColTab;
    f.a = __popc(m.plain & below(i));
    f.b = fold<uint32_t>(0u, m.tab, m.plain, i + 1u, 16u, tm);
  } else {  // the common granule
    f.kind = kColAdd;
    f.a = __popc(m.plain);
  }
  return f;
}

}  // namespace

__global__ __launch_bounds__(kSWaves * 64) void col_summary_kernel(ColParams C)
{
  const int lane = threadIdx.x & 63;
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (gw >= C.nwaves) return;
  const SRange r = srange(C.len, C.per, gw);
  const uint32_t tm = C.tmask;
  ColFn R{};          // the range so far
  uint32_t cnt = 0;   // newlines, per lane
  uint32_t last = 0;  // 1 + range offset of the lane's last newline
  for (uint32_t i = 0; i < r.n; ++i) {
    const __amdgpu_buffer_rsrc_t rs = ltile(C.g + r.lo, i, r.rel16);
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = sload16(rs, 64u * lane + 16u * k);
    ColFn T{};  // the lane's 64 bytes
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t ro = i * (uint32_t)kSTile + 64u * lane + 16u * k;
      const GMasks m = granule_masks(v[k], granule_valid(r.rel, ro));
      cnt += __popc(m.nl);
      if (m.nl) last = ro + 32u - (uint32_t)__builtin_clz(m.nl);
      T = compose(T, granule_fn(m, tm), tm);
    }
    R = compose(R, fn_lane63(fn_scan(T, tm)), tm);
  }
  const uint64_t t = wave_sum((uint64_t)cnt);
  const uint64_t l = wave_max((uint64_t)last);
  if (lane == 0) {
    C.counts[gw] = t;
    C.lastnl[gw] = l ? r.lo + l : 0ull;
    C.fn_a[gw] = (uint64_t)R.a | ((uint64_t)R.kind << 32);
    C.fn_b[gw] = R.b;
  }
}

__global__ __launch_bounds__(kSWaves * 64) void col_assign_kernel(ColParams C)
{
  // per granule g of the tile (lane g / 4 loads granules 4 lane .. 4 lane + 3):
  // its masks, and what holds at its first byte: the newlines of the tile
  // before it, 1 + tile offset of the last of them, and the column function of
  // the tile's bytes before it
  __shared__ uint16_t gnl[kSWaves][256], gtab[kSWaves][256], gplain[kSWaves][256], gpre[kSWaves][256],
      glast[kSWaves][256];
  __shared__ uint32_t fkind[kSWaves][256], fa[kSWaves][256], fb[kSWaves][256];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t gw = (uint64_t)blockIdx.x * kSWaves + wid;
  if (gw >= C.nwaves) return;
  const SRange r = srange(C.len, C.per, gw);
  const uint32_t tm = C.tmask;
  const bool lastw = gw == C.nwaves - 1;  // it also takes the positions >= len
  uint64_t j = lower64(C.pos, C.npos, r.lo, lane);  // next position to assign
  uint64_t line = 1 + C.prefix[gw];  // at the tile's first byte: its line, the line's begin, its column
  uint64_t bol = C.bol[gw];
  uint64_t kin = C.kin[gw];
  for (uint32_t i = 0; i < r.n && j < C.npos; ++i) {
    wave_sync();  // the previous tile's LDS reads precede these writes
    const uint64_t ts = r.lo + (uint64_t)i * kSTile;
    const __amdgpu_buffer_rsrc_t rs = ltile(C.g + r.lo, i, r.rel16);
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = sload16(rs, 64u * lane + 16u * k);
    // within the lane's 64 bytes, before granule k: function, newlines, last newline
    ColFn e[4], T{};
    uint32_t cpre[4], lpre[4], cl = 0, ll = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t g = 4u * lane + k;
      const GMasks m = granule_masks(v[k], granule_valid(r.rel, i * (uint32_t)kSTile + 16u * g));
      gnl[wid][g] = (uint16_t)m.nl;
      gtab[wid][g] = (uint16_t)m.tab;
      gplain[wid][g] = (uint16_t)m.plain;
      e[k] = T, cpre[k] = cl, lpre[k] = ll;
      T = compose(T, granule_fn(m, tm), tm);
      cl += __popc(m.nl);
      if (m.nl) ll = 16u * g + 32u - (uint32_t)__builtin_clz(m.nl);
    }
    // across the lanes: the same three before the lane's first byte
    const ColFn incl = fn_scan(T, tm);
    const uint32_t inclc = lscan_add(cl), inclp = lscan_max(ll);
    // (every lane takes part in the shuffles; lane 0 then drops what it got)
    const uint32_t uk = __shfl_up(incl.kind, 1, 64), ua = __shfl_up(incl.a, 1, 64), ub = __shfl_up(incl.b, 1, 64);
    const uint32_t up = __shfl_up(inclp, 1, 64);
    ColFn X;
    X.kind = lane ? uk : (uint32_t)kColAdd, X.a = lane ? ua : 0u, X.b = lane ? ub : 0u;
    const uint32_t exclp = lane ? up : 0u, exclc = inclc - cl;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t g = 4u * lane + k;
      const ColFn f = compose(X, e[k], tm);
      gpre[wid][g] = (uint16_t)(exclc + cpre[k]);
      glast[wid][g] = (uint16_t)umax(exclp, lpre[k]);
      fkind[wid][g] = f.kind, fa[wid][g] = f.a, fb[wid][g] = f.b;
    }
    const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int)inclc, 63);
    const uint32_t lastp = (uint32_t)__builtin_amdgcn_readlane((int)inclp, 63);
    const ColFn F = fn_lane63(incl);
    wave_sync();
    const uint64_t tend = ts + kSTile < r.hi ? ts + kSTile : r.hi;
    for (;;) {  // positions in this tile, 64 at a time
      const uint64_t idx = j + (uint64_t)lane;
      const uint64_t s = idx < C.npos ? C.pos[idx] : ~0ull;
      const bool in = s < tend;
      const uint64_t mb = __ballot(in);
      if (!mb) break;
      if (in) {
        const uint32_t x = (uint32_t)(s - ts), g = x >> 4, t = x & 15u;
        const uint32_t nlm = gnl[wid][g], tabm = gtab[wid][g], plain = gplain[wid][g];
        const uint32_t before = nlm & below(t);  // newlines of the granule before the position
        uint64_t b, c;
        if (before) {
          const uint32_t sb = 32u - (uint32_t)__builtin_clz(before);
          b = ts + 16u * g + sb;
          c = fold<uint64_t>(0ull, tabm, plain, sb, t, tm);
        } else {
          const uint32_t lp = glast[wid][g];
          ColFn f;
          f.kind = fkind[wid][g], f.a = fa[wid][g], f.b = fb[wid][g];
          b = lp ? ts + lp : bol;
          c = fold<uint64_t>(apply(f, kin, tm), tabm, plain, 0u, t, tm);
        }
        if (C.col) C.col[idx] = c;
        if (C.bolout) C.bolout[idx] = b;
        if (C.line) C.line[idx] = line + (uint32_t)gpre[wid][g] + __popc(before);
      }
      const uint32_t k = (uint32_t)__popcll(mb);
      j += k;
      if (k < 64) break;
    }
    line += base;
    if (lastp) bol = ts + lastp;
    kin = apply(F, kin, tm);
    if (j >= C.npos) break;
    const uint64_t nxt = C.pos[j];
    if (lastw ? nxt > r.hi : nxt >= r.hi) break;  // no further position in this range
  }
  if (!lastw) return;
  // position len takes what holds behind the last byte (every tile was walked
  // when one is left); larger ones do not exist
  for (uint64_t idx = j + (uint64_t)lane; idx < C.npos; idx += 64) {
    const bool at = C.pos[idx] == C.len;
    if (C.col) C.col[idx] = at ? kin : ~0ull;
    if (C.bolout) C.bolout[idx] = at ? bol : ~0ull;
    if (C.line) C.line[idx] = at ? line : ~0ull;
  }
}

hipError_t launch_col_summary(const ColParams& C, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((C.nwaves + kSWaves - 1) / kSWaves);
  hipLaunchKernelGGL(col_summary_kernel, dim3(grid), dim3(kSWaves * 64), 0, stream, C);
  return hipGetLastError();
}

hipError_t launch_col_assign(const ColParams& C, hipStream_t stream)
{
  const uint32_t grid = (uint32_t)((C.nwaves + kSWaves - 1) / kSWaves);
  hipLaunchKernelGGL(col_assign_kernel, dim3(grid), dim3(kSWaves * 64), 0, stream, C);
  return hipGetLastError();
}

}  // namespace ugpu

// ---------------------------------------------------------------- C ABI
using namespace ugpu;

int ugpu_columns(const uint8_t* dbuf, uint64_t len, const uint64_t* d_pos, uint64_t n, uint32_t tab, uint64_t* d_col,
                 uint64_t* d_bol, uint64_t* d_line, void* stream)
{
  if (tab != 1 && tab != 2 && tab != 4 && tab != 8) return fail(UGPU_INVAL, "tab size must be 1, 2, 4 or 8");
  if (!d_col && !d_bol && !d_line) return fail(UGPU_INVAL, "no output array");
  if (!dbuf || (n && !d_pos)) return fail(UGPU_INVAL, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dbuf) & 15u) return fail(UGPU_INVAL, "buffer must be 16-byte aligned");
  if (!n) return UGPU_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint64_t per = 0, nw = 0;
  const int dev = line_wave_ranges(len, &per, &nw);
  if (dev < 0) return UGPU_DEVICE;
  WsLease<WaveWs> ws(dev);
  if (!ws.ws) return fail(UGPU_NOMEM, "columns workspace");
  hipError_t e = ws->reserve(nw, 4);
  if (e != hipSuccess) return hip_fail(e, "columns buffers");
  ColParams C{};
  C.g = dbuf;
  C.len = len;
  C.per = per;
  C.nwaves = nw;
  C.tmask = tab - 1;
  C.pos = d_pos;
  C.npos = n;
  C.counts = ws->d_out;
  C.lastnl = ws->d_out + nw;
  C.fn_a = ws->d_out + 2 * nw;
  C.fn_b = ws->d_out + 3 * nw;
  C.prefix = ws->d_in;
  C.bol = ws->d_in + nw;
  C.kin = ws->d_in + 2 * nw;
  C.col = d_col;
  C.bolout = d_bol;
  C.line = d_line;
  if ((e = launch_col_summary(C, st)) != hipSuccess ||
      (e = hipMemcpyAsync(ws->h_out, ws->d_out, nw * 4 * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "column summary");
  column_stitch(ws->h_out, ws->h_in, nw, C.tmask);
  if ((e = hipMemcpyAsync(ws->d_in, ws->h_in, nw * 3 * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = launch_col_assign(C, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
    return hip_fail(e, "column assignment");
  return UGPU_OK;
}
