// switches.h — the A/B switches of the library.  Plain C++ (no HIP): conv_plan.h reads them and must compile on a host compiler alone.
#pragma once
#include <cstdlib>

namespace lrp {

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
  int conv_breg2 = 1;       // LRP_CONV_BREG2=0    the N <= 64 weights-in-registers launches of the dense split-bf16 walk (FORM_BREG) on their first loop
                            //                     (whole fragment sets double-buffered, a full stop between channel groups) instead of the chunk loop; a per-launch switch only
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
    if (const char* e = getenv("LRP_CONV_BREG2")) conv_breg2 = atoi(e);   // (likewise: tests/test_gpu_conv_breg2.py)
    if (const char* e = getenv("LRP_CONV_SPARSE_WREG")) conv_sparse_wreg = atoi(e);   // (likewise: tests/test_gpu_conv_sparse_wreg.py)
  }
};
inline Switches& sw() {
  static Switches s = [] { Switches t; t.load(); return t; }();
  return s;
}

}  // namespace lrp
