// hip_host.hpp -- host-side HIP plumbing of the engine (engine.hip, utf8.hip,
// gen.hip, and through line_host.hpp the line calls): error reporting, the
// owning device / pinned arrays, the table upload, and the per-device
// workspace pool.  Every hipMalloc / hipFree / hipHostMalloc / hipHostFree of
// the library is here, but for the size-classed pinned block cache of
// engine.hip (pinned_get / pinned_put).
//
// Process exit: nothing is freed once the process is ending (engine.hip
// exiting()).  The release calls return before they delete an owner, the pools
// hold raw pointers and are never torn down, and no object with static storage
// duration may hold a HipBuf by value.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ugpu.h"
#include "plan.hpp"

namespace ugpu {

// (the error string lives in the host library, libugpu_host.so: ugpu_last_error)
inline int fail(int code, const std::string& msg) { return host_fail(code, msg); }

inline int hip_fail(hipError_t e, const char* what)
{
  return host_fail(UGPU_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                              \
  do {                                             \
    hipError_t _e = (expr);                        \
    if (_e != hipSuccess) return hip_fail(_e, #expr); \
  } while (0)

inline bool is_device_ptr(const void* p)
{
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

// An owning array of cap elements of T in device memory (PIN: pinned host
// memory), move-only, freed by its destructor.  It converts to its pointer;
// null means "none".  The caller of reserve() passes the capacity to allocate,
// so every site keeps its own growth rule; `pad` elements are allocated beyond
// cap and not counted (16 bytes behind inputs the kernels read in 16-byte
// loads).  A failed alloc() or reserve() leaves the array empty.
template <class T, bool PIN>
struct HipBuf {
  T* p = nullptr;
  uint64_t cap = 0;  // elements

  HipBuf() = default;
  ~HipBuf() { release(); }
  HipBuf(HipBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  HipBuf& operator=(HipBuf&& o) noexcept
  {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  operator T*() const { return p; }
  T* operator->() const { return p; }

  void release()
  {
    if (p) (void)(PIN ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  // exactly n elements, replacing what it held
  hipError_t alloc(uint64_t n, uint64_t pad = 0)
  {
    release();
    const size_t bytes = (n + pad) * sizeof(T);
    const hipError_t e = PIN ? hipHostMalloc(reinterpret_cast<void**>(&p), bytes) : hipMalloc(&p, bytes);
    if (e != hipSuccess)
      p = nullptr;
    else
      cap = n;
    return e;
  }
  // room for `need` elements: grows (contents lost) to new_cap elements
  hipError_t reserve(uint64_t need, uint64_t new_cap, uint64_t pad = 0)
  {
    return need <= cap ? hipSuccess : alloc(new_cap, pad);
  }
  // reserve() that keeps the first `keep` elements: the new block is allocated
  // first, the elements are copied on `st`, which is synchronised, and then the
  // old block is freed.  On failure the array stays as it was.
  hipError_t reserve_keep(uint64_t need, uint64_t new_cap, uint64_t keep, hipStream_t st, uint64_t pad = 0)
  {
    static_assert(!PIN, "device arrays only");
    if (need <= cap) return hipSuccess;
    if (!keep) return alloc(new_cap, pad);
    HipBuf nb;
    hipError_t e = nb.alloc(new_cap, pad);
    if (e == hipSuccess) e = hipMemcpyAsync(nb.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) *this = std::move(nb);
    return e;
  }
  // the table upload: exactly n0 + n1 elements, a[0, n0) then b[0, n1) copied from the host
  hipError_t upload(const T* a, size_t n0, const T* b = nullptr, size_t n1 = 0)
  {
    static_assert(!PIN, "device arrays only");
    hipError_t e = alloc(n0 + n1);
    if (e == hipSuccess) e = hipMemcpy(p, a, n0 * sizeof(T), hipMemcpyHostToDevice);
    if (e == hipSuccess && n1) e = hipMemcpy(p + n0, b, n1 * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
};
template <class T>
using DevBuf = HipBuf<T, false>;
template <class T>
using PinBuf = HipBuf<T, true>;

// w.init() where W has one (the streams and events of a new workspace)
template <class W>
auto ws_init(W& w, int) -> decltype(w.init())
{
  return w.init();
}
template <class W>
hipError_t ws_init(W&, long)
{
  return hipSuccess;
}

// A workspace of type W (with an int dev) taken from the idle ones of its
// device, so that repeated calls do no hipMalloc or hipFree (hipFree
// synchronises the device): for the length of a call (the lease), or with
// take() / give() by an owner that keeps it across calls.  A new workspace
// runs its init(), if it has one, and is destroyed again when that fails.
// Idle workspaces are kept for the process lifetime.  ws (take()) is NULL when
// none could be made.
template <class W>
struct WsLease {
  W* ws = nullptr;

  explicit WsLease(int dev) : ws(take(dev)) {}
  ~WsLease() { give(ws); }
  WsLease(const WsLease&) = delete;
  WsLease& operator=(const WsLease&) = delete;
  W* operator->() const { return ws; }

  static W* take(int dev)
  {
    Pool& p = pool();
    {
      std::lock_guard<std::mutex> lk(p.mu);
      for (size_t i = 0; i < p.idle.size(); ++i)
        if (p.idle[i]->dev == dev) {
          W* w = p.idle[i];
          p.idle.erase(p.idle.begin() + (long)i);
          return w;
        }
    }
    W* w = new (std::nothrow) W;
    if (!w) return nullptr;
    w->dev = dev;
    if (ws_init(*w, 0) != hipSuccess) {
      delete w;
      return nullptr;
    }
    return w;
  }
  static void give(W* w)
  {
    if (!w) return;
    Pool& p = pool();
    std::lock_guard<std::mutex> lk(p.mu);
    p.idle.push_back(w);
  }

 private:
  struct Pool {
    std::mutex mu;
    std::vector<W*> idle;
  };
  static Pool& pool()
  {
    static Pool& p = *new Pool;  // (never destroyed: releases may come from static destructors)
    return p;
  }
};

}  // namespace ugpu
