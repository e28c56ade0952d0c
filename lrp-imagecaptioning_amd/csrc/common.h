// common.h — error plumbing and small RAII helpers shared by the engine sources.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/lrp_hip.h"
#include "switches.h"

namespace lrp {

// Every kernel launch of the library goes through hipLaunchKernelGGL; this wrapper counts them (lrp_launch_count: bench.py
// reports the launches behind one single-image explanation next to its latency).  Memsets / copies are not counted.
// (atomic, relaxed: handles may be driven from several host threads — bench.py's power probe does)
inline std::atomic<unsigned long long> g_launch_count{0};
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, numBlocks, numThreads, memPerBlock, streamId, ...)                  \
  do {                                                                                                    \
    ::lrp::g_launch_count.fetch_add(1, std::memory_order_relaxed);                                       \
    kernelName<<<(numBlocks), (numThreads), (memPerBlock), (streamId)>>>(__VA_ARGS__);                   \
  } while (0)

std::string& last_error_ref();

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error_ref() = buf;
  return code;
}

#define LRP_HIP_CHECK(expr)                                                                     \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return ::lrp::fail(LRP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                         __FILE__, __LINE__);                                                   \
  } while (0)

#define LRP_TRY(expr)         \
  do {                        \
    int _rc = (expr);         \
    if (_rc != LRP_OK) return _rc; \
  } while (0)

// Device allocation owned by the handle (workspace); freed in the destructor.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool owned = true;                                   // false: a window of another DevBuf (view_of), never freed here
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), owned(o.owned) { o.p = nullptr; o.bytes = 0; o.owned = true; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; bytes = o.bytes; owned = o.owned; o.p = nullptr; o.bytes = 0; o.owned = true; }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    owned = true;
  }
  // n bytes at `offset` of `arena` (which must outlive this view)
  void view_of(const DevBuf& arena, size_t offset, size_t n) {
    release();
    p = static_cast<char*>(arena.p) + offset;
    bytes = n;
    owned = false;
  }
  int alloc(size_t n, int64_t* total) {
    release();
    if (n == 0) n = 16;
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();                         // clear the sticky error: the next launch check must not report this one
      return fail(LRP_ERR_NOMEM, "device memory: hipMalloc(%zu bytes) failed: %s", n, hipGetErrorString(e));
    }
    bytes = n;
    if (total) *total += (int64_t)n;
    return LRP_OK;
  }
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// Per-launch timing of the reverse walks (lrp_profile_enable / _query / _records): a pair of events around a launch and the
// algorithmic flops booked on it.  Off: begin / end do nothing and the list stays empty.
struct ProfileRec {
  hipEvent_t e0, e1;
  double flop;
};
struct Profiler {
  bool on = false;
  ProfileRec cur{};                                    // between begin and end
  std::vector<ProfileRec> recs;
  void begin(hipStream_t st) {
    if (on) { (void)hipEventCreate(&cur.e0); (void)hipEventCreate(&cur.e1); (void)hipEventRecord(cur.e0, st); }
  }
  void end(hipStream_t st, double flop) {
    if (on) { (void)hipEventRecord(cur.e1, st); cur.flop = flop; recs.push_back(cur); }
  }
  // waits for every record, hands (ms, flop) of those that finished to `each`, and empties the list
  template <typename F>
  void drain(F each) {
    for (ProfileRec& p : recs) {
      float t = 0.f;
      if (hipEventSynchronize(p.e1) == hipSuccess && hipEventElapsedTime(&t, p.e0, p.e1) == hipSuccess) each((double)t, p.flop);
      (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1);
    }
    recs.clear();
  }
  int records(int cap, double* ms_out, double* flop_out, int* n_out) {
    int k = 0;
    drain([&](double ms, double flop) { if (k < cap) { ms_out[k] = ms; flop_out[k] = flop; ++k; } });
    *n_out = k;
    return LRP_OK;
  }
  int query(int64_t* launches, double* ms, double* flop) {
    int64_t nl = 0; double tm = 0, fl = 0;
    drain([&](double t, double f) { tm += t; fl += f; ++nl; });
    if (launches) *launches = nl;
    if (ms) *ms = tm;
    if (flop) *flop = fl;
    return LRP_OK;
  }
};

}  // namespace lrp
