// fwd_mode.h — which forward Encoder::encode runs.  A pure function of the precision, the layer widths and what the weight
// packing left; no HIP in here, so tests/test_fwd_mode.py builds it into a stand-alone program.
#pragma once
#include <cstddef>

namespace lrp {

// FWD_EXACT: dual fp32 GEMM per layer, gate or pool-gate pass behind it (Encoder::forward_exact)
// FWD_PAIRS: a_l | Z+_l in one pass on fp16 pairs (forward_pairs_emit / forward_pairs_split): the default; emit: pairs, gates and
//            maxima leave the conv / pool epilogues, one scale per image
// FWD_FAST : split-bf16 activation chain, Z+ and the gates on the side stream (forward_fast)
enum FwdMode { FWD_EXACT, FWD_PAIRS, FWD_FAST };
struct FwdPlan { FwdMode mode; bool emit; };

// bf16x3: every precision but LRP_PREC_FP32; fast: LRP_PREC_BF16X3_FAST.  Split operands come in groups of 8 channels, and the
// side stream has nothing to overlap with in a one-layer net: exact fp32 there.  cin of layer l is cout of layer l - 1, so the
// output widths are all there is to ask.
// emit_ready: LRP_FWD_EMIT is on, every layer was packed with interleaved rows (Encoder::dual_interleaved: LRP_FWD_IL and
// cout % 32 == 0) and an image has a multiple of four floats; the image layer's epilogue cannot pool, hence pool_after0.
inline FwdPlan forward_mode(bool bf16x3, bool fast, const int* cout, size_t n_layers, bool pool_after0, bool emit_ready) {
  bool mixed = bf16x3 && n_layers > 1;
  for (size_t li = 0; li < n_layers; ++li)
    if (cout[li] & 7) mixed = false;
  if (!mixed) return {FWD_EXACT, false};
  if (fast) return {FWD_FAST, false};
  return {FWD_PAIRS, emit_ready && !pool_after0};
}

}  // namespace lrp
