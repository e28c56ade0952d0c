// encoder_state.h — what the analyzers of the VGG encoder keep on a handle, one struct per role header: the rule table
// (encoder_rules.h), DeepLIFT (encoder_deeplift.h), the layer trace (encoder_trace.h), PatternNet / PatternAttribution
// (encoder_pattern.h).  Encoder owns one of each; their per-layer records are sized in Encoder::init and indexed like
// Encoder::layers.  Every buffer here is allocated by the first call of its analyzer that needs it: a handle that never uses an
// analyzer pays nothing for it, and neither ConvLayer nor the hot path's switches carry any of it.
#pragma once
#include <algorithm>
#include <vector>
#include "common.h"

namespace lrp {
// One conv's rule (lrp_set_cnn_rule, lrp_set_cnn_rules)
struct ConvRule {
  int kind = LRP_RULE_ALPHA_BETA, bias = 1;
  float alpha = 1.f, beta = 0.f, eps = 0.f, low = 0.f, high = 0.f;
  int chains() const { return kind == LRP_RULE_ALPHA_BETA && beta > 0.f ? 2 : 1; }
  bool own_gate() const { return kind != LRP_RULE_ALPHA_BETA || !bias; }       // activator gate not the forward's a / safe(Z+)
  bool fwd_a() const { return (kind == LRP_RULE_ALPHA_BETA && !bias) || kind == LRP_RULE_BOUNDED; }   // ... and its denominator a conv with w+ | w-
  bool input_only() const { return kind == LRP_RULE_FLAT || kind == LRP_RULE_WSQUARE || kind == LRP_RULE_BOUNDED; }
  // does a layer under this rule walk on the default walk's own backward matrix (w+ tap-flipped; the image layer: w+ ; w-)?
  bool on_default_matrix() const { return kind == LRP_RULE_ALPHA_BETA && bias && chains() == 1; }
  // what the image layer's stencil selects (cnn_kernels.h img_stencil_kernel): x+ / x- | x | x with epsilon's sign | x - low / x - high
  int img_mode() const { return kind == LRP_RULE_ALPHA_BETA ? 0 : kind == LRP_RULE_EPSILON ? 2 : kind == LRP_RULE_BOUNDED ? 3 : 1; }
};

struct RuleTableState {
  // The handle's rule.  Empty: the default alpha1beta0 walk with all its fast forms — nothing below is allocated, launched or read.
  // Anything else, the same (alpha, beta > 0, bias) record on every conv (the one-rule entry) included, is a table.
  std::vector<ConvRule> table;
  // Per conv: the activator gate of a rule whose denominator is not the forward's Z+, the forward matrix of that denominator (fp32,
  // split8) and the layer's backward matrix over its one or two chains (cnn_kernels.h pack_conv_rule_dev_kernel /
  // pack_image_layer_rule_dev_kernel); for alpha-beta with beta > 0 the inhibitor gate G- = a / safe(Z_inh) next to G (same mask)
  // and the forward matrix w- of its denominator conv (fp32, split8).
  struct Layer { DevBuf Gt, w_fwd_t, w_fwd_ts, w_bwd_t, w_bwd_t_s, Gn, w_fwd_n, w_fwd_ns; bool packed = false; };
  std::vector<Layer> layer;
  DevBuf zt_top, wsq_zc;                               // the top layer's activator denominator where it is not ztop; w-square's border classes
  DevBuf a1b;                                          // BoundedRule: im2col of the image layer over (x - low | x - high) — a1 stays the forward's (the fine-tune step reads it)
  DevBuf zntop, s0ab, s1ab;                            // two chains: Z_inh of the top layer; the two-chain ping-pong
  bool on() const { return !table.empty(); }
  bool has_eps() const { return std::any_of(table.begin(), table.end(), [](const ConvRule& r) { return r.kind == LRP_RULE_EPSILON; }); }
  static int chains_of(const std::vector<ConvRule>& t) { return std::any_of(t.begin(), t.end(), [](const ConvRule& r) { return r.chains() == 2; }) ? 2 : 1; }
};

struct DeepLiftState {
  // Per conv: the reference's input and activation of this layer — ONE image's worth, from the reference's own forward — and per
  // image the gate D = M ? safe(Y - Yr) : 0 (deeplift_kernels.h dl_gate_kernel; every layer, the top one included)
  struct Layer { DevBuf Xr, Yr, Dl; };
  std::vector<Layer> layer;
  int mode = 0;                                        // 0 off | 1 approximate_gradient=False (one chain) | 2 True (two chains + select)
  bool ref_stale = true, capture = false;              // capture: the forward that runs is the reference's (Encoder::dual_fp32_layer keeps Xr / Yr)
  long epoch = -1;                                     // the encode whose gates D_l are current
  std::vector<float> ref_host;                         // the reference as set, broadcast to (img_h, img_w, 3)
  DevBuf s0, s1, r2i;                                  // mode 2: the two chains' ping-pong (2 max_tokens rows) and row2img twice
};

struct TraceTensor {
  int nid, H, W, C;
  size_t elems() const { return (size_t)H * W * C; }
};
struct TraceState {
  bool on = false;                                     // lrp_set_layer_trace: while it is on the handle keeps every conv's input
  DevBuf part;                                         // [2 tensors][max_tokens][chunks of the largest layer][TRACE_PART] doubles
};

struct PatternState {
  // Per conv: the fit's float64 sums [Sx | Sxy | cnt | Sy | P], the pattern A (HWIO, as fitted or as set) and its packed copies for
  // the walk's transposed conv — A and A * w in w_bwd_full's layout, rebuilt by the next pattern walk after the pattern or the
  // weights changed
  struct Layer { DevBuf sums, A, bwd, bwd_w; bool have = false, packed = false; };
  std::vector<Layer> layer;
  static size_t sum_doubles(int cin, int cout) { return (size_t)2 * 9 * cin * cout + 2 * (size_t)cout + 1; }
  int type = -1;                                       // the running fit's mask (PAT_*), -1: no fit is open
  long fit_epoch = -1, batches = 0;                    // the encode accumulated last; batches accumulated by this fit
  bool project = true;                                 // reverse_project_bottleneck_layers (pattern_based.py:175-183)
  DevBuf prod, ws, part;                               // fit: the batch's two products (fp32), the K-split workspace, the mask pass' partials
  size_t ws_floats = 0;
  DevBuf div, maxpart;                                 // walk: a row's divisor, the partials of its maximum
};

}  // namespace lrp
