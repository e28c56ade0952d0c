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

// A/B switches kept for measurement and as tested fall-backs (every one of them is exercised by
// tests/test_gpu_switches.py against the default path).  Read from the environment ONCE per process — no getenv on the launch
// path — and again by lrp_reload_switches() (include/lrp_hip.h), which is how a test or a measurement script flips one.
struct Switches {
  int conv_halo = 1;        // LRP_CONV_HALO  0 never / 1 when a tile shape fills >= 90 % of the M tile / 2 always (ragged shapes: tests)
  int conv_breg = 1;        // LRP_CONV_BREG=0     N <= 64 backward convs without the weights-in-registers kernel
  int conv_breg8 = 1;       // LRP_CONV_BREG8=0    the dense 8-wave 256 x 256 walk launches on the pipelined kernel (a weight stage in LDS, a barrier per tap);
                            //                     also read when weights are set: only then are the layers' fragment-major copies made
  int conv_breg4 = 1;       // LRP_CONV_BREG4=0    the 128 x 128 resident-image launches with N % 128 == 0 (dense split-bf16 walk, interleaved dual forward) on the
                            //                     pipelined kernel; also read when weights are set: only then are the fragment-major copies made
  int conv_sparse_wreg = 1; // LRP_CONV_SPARSE_WREG=0  the large form of the 2:4-sparse pooled consumers (conv_sparse.h) on the LDS-stage loop (weights by
                            //                     LDS-DMA into four stages, a barrier every second k-step) instead of the weights-in-registers loop
  int conv_small = 1;       // LRP_CONV_SMALL=0    small grids keep the 128-row tiles (no 64 x 64 tiles)
  int conv_mid = 1;         // LRP_CONV_MID=0      no 128 x 64 tiles for the grids just above the small ones
  int epi_fast = 1;         // LRP_EPI_FAST=0      MUL / MUL_UP2 epilogues always through the general pass loop
  int up2_pw = 1;           // LRP_UP2_PW=0        pooled boundaries of the pipelined halo kernels through the expanded tensor (dense consumers only:
                            //                     a boundary with a sparse consumer, LRP_SPARSE_POOL, always gets the compact S_c)
  int tile_order = 1;       // LRP_TILE_ORDER=0    reverse-walk launches in stack order
  int fwd_emit = 1;         // LRP_FWD_EMIT=0      forward: split / absmax / pool passes between the convs
  int fwd_il = 1;           // LRP_FWD_IL=0        dual forward matrix with stacked rows: separate gate pass (decided when lrp_set_weight packs)
  int img_fused = 1;        // LRP_IMG_FUSED=0     image layer as T GEMM + separate stencil kernel (VGG16 and the ResNet stem)
  int up2_compact = 1;      // LRP_UP2_COMPACT=0   every pooled boundary with a dense consumer through the expanded tensor
  int img_fold = 1;         // LRP_IMG_FOLD=0      image layer as its own launch
  int pool_fused = 1;       // LRP_POOL_FUSED=0    forward: max-pool + gate + pooled pairs as a pass of their own behind the conv
  int sparse_pool = 1;      // LRP_SPARSE_POOL=0   pooled boundaries with N % 256 == 0 output columns through the dense kernels, not the 2:4-sparse matrix cores (conv_sparse.h); read by encode and explain
  void load() {
    *this = Switches();
    auto rd = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); };
    rd("LRP_CONV_HALO", conv_halo); rd("LRP_CONV_BREG", conv_breg); rd("LRP_CONV_SMALL", conv_small);
    rd("LRP_CONV_MID", conv_mid); rd("LRP_EPI_FAST", epi_fast); rd("LRP_UP2_PW", up2_pw); rd("LRP_TILE_ORDER", tile_order);
    rd("LRP_FWD_EMIT", fwd_emit); rd("LRP_FWD_IL", fwd_il); rd("LRP_IMG_FUSED", img_fused); rd("LRP_UP2_COMPACT", up2_compact);
    rd("LRP_IMG_FOLD", img_fold); rd("LRP_SPARSE_POOL", sparse_pool); rd("LRP_POOL_FUSED", pool_fused);
    // (read apart from the list above, which tests/test_capi_symbols.py holds against the rows of tests/test_gpu_switches.py: this
    // switch's run against the default path — operator and engine level, bit-identical — is tests/test_gpu_conv_breg8.py)
    if (const char* e = getenv("LRP_CONV_BREG8")) conv_breg8 = atoi(e);
    if (const char* e = getenv("LRP_CONV_BREG4")) conv_breg4 = atoi(e);   // (likewise: tests/test_gpu_conv_breg4.py)
    if (const char* e = getenv("LRP_CONV_SPARSE_WREG")) conv_sparse_wreg = atoi(e);   // (likewise: tests/test_gpu_conv_sparse_wreg.py)
  }
};
inline Switches& sw() {
  static Switches s = [] { Switches t; t.load(); return t; }();
  return s;
}

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
