// encoder.h — host-side orchestration of the CNN half (VGG): struct Encoder, one translation unit, one header per role.
//   encoder.h           ConvLayer (the forward's and the default walk's operands), the handle's core state, init(), the users of
//                       the kept activations, encode() (one forward per IMAGE, caching the relevance gates G_l and Z_top), WalkMode,
//                       the step helpers every walk shares, and explain(): one reverse walk per TOKEN (batched over all tokens of
//                       the call) — the default LRP walk and the gradient family (walk = 1..4).  The hot path.
//   encoder_state.h     ConvRule and what each analyzer keeps on the handle: RuleTableState, DeepLiftState, TraceState, PatternState
//   encoder_weights.h   the device packers: alloc_conv_operands, repack_*, set_conv_*_dev
//   encoder_forward.h   the four forward paths (exact, fast, pairs split, pairs emit) and their launch helpers
//   encoder_rules.h     the rule table: set_table, pack_table_layer, table_pass, rule_head, explain_table
//   encoder_deeplift.h  DeepLIFT: set_deeplift_reference, dl_reference_pass, dl_pass, explain_deeplift
//   encoder_trace.h     the layer trace: set_layer_trace, trace_tensors / trace_keep_layout, explain_traced
//   encoder_pattern.h   PatternNet / PatternAttribution: pattern_fit_*, pattern_set, pattern_pack, explain_pattern
// The role headers define what struct Encoder declares (inline int Encoder::...); they are included at the bottom of this file.
// Reference semantics: LRPSequentialPresetA.analyze([X,R]) (AB:478-520) over the
// sub-model input_1 -> block5_conv3 (E:29-32); rules RR:274-322, RA:470-480.
#pragma once
#include <algorithm>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "cnn_kernels.h"
#include "common.h"
#include "conv_launch.h"
#include "conv_plan.h"
#include "conv_sparse.h"
#include "deeplift_kernels.h"
#include "encoder_state.h"
#include "f16_operand.h"
#include "fwd_mode.h"
#include "pattern_kernels.h"
#include "trace_kernels.h"
#include "train_gemm.h"

namespace lrp {

struct ConvLayer {
  std::string name;
  int cin = 0, cout = 0, H = 0, W = 0;   // H,W = resolution this conv runs at
  bool pool_after = false;
  bool have_w = false, have_b = false;
  DevBuf w_fwd;    // dual-packed forward weights  (a_l | Z+_l)          [fp32 mode, and the image layer]
  DevBuf w_fwd_a;  // forward weights w, fp32                            [mixed mode: exact activation conv]
  DevBuf w_fwd_zs; // forward weights w+, split8                         [mixed mode: bf16x3 denominator conv]
  DevBuf w_fwd_as; // forward weights w, split8                                    [activation conv, LRP_PREC_BF16X3_FAST]
  DevBuf w_fwd_h;  // the dual matrix (w | w+) of w_fwd as fp16 pairs, one common scale (record wds)   [a_l and Z+_l in one pass, default]
  DevBuf wds;
  DevBuf w_bwd;    // w+ (and w- for the image layer), tap-flipped, packed for convT-as-conv
  DevBuf w_bwd_s;  // the same matrix in split8 (bf16 hi|lo) form for the bf16x3 reverse walk
  DevBuf w_bwd_full;  // full w (both signs), tap-flipped: the gradient baselines' backward-data conv (fp32)
  DevBuf w_bwd_full_s;  // the same in split8 form: backward-data conv of the fine-tune step on the bf16 matrix cores
  DevBuf w_bwd_h;     // w_bwd in fp16 split8 form [hi8 | lo8] (PREC_F16X2 reverse walk: only hi is read), and ...
  DevBuf w_bwd_frag_h;   // ... fragment-major for the weights-in-registers kernel
  DevBuf wbs;         // device record {2^k, 2^-k, norm, k} of the fp16 backward copy's power-of-two scale
  DevBuf w_fwd_il;    // the dual forward matrix with its rows interleaved per 32 channels ([w | w+] side by side): fp32 source of w_fwd_h
  std::unique_ptr<TileOrder> order{new TileOrder};   // tile-row order of this layer's reverse launch (conv_args.h)
  DevBuf w_bwd_frag;  // w_bwd_s fragment-major: layers whose backward conv can take a weights-in-registers kernel (conv_plan.h conv_frag_forms)
  DevBuf w_fwd_frag;  // w_fwd_h fragment-major: interleaved layers whose dual forward can (the same function)
  DevBuf bias;
  DevBuf G;        // [max_images][H][W][cout] relevance gate (not for the top layer)
  DevBuf P;        // [max_images][H/2][W/2][cout] pooled activations (pool_after layers; overlapped encode)
  // the gate of a pooled layer in COMPACT form (value + position per window and channel), for the consumer of the compact
  // pool interface; written by pool_gate_split_kernel, valid for the encode whose number gc_epoch holds
  DevBuf Gc, Gpos;
  long gc_epoch = -1;
  // the full-resolution gate G of a pooled layer is current for the encode whose number this holds: the fused pool epilogue
  // writes the compact form only, Encoder::full_gate() expands it for the walks that read G (cnn_kernels.h pool_gate_expand_kernel)
  long gfull_epoch = -1;
  // Deconvnet walk (LRP_WALK_DECONVNET): the pool's routing alone as a 0/1 gate at full resolution — 1 at the forward's arg-max
  // cell of every window, the FIRST cell in scan order where the whole window is zero (G is zero there and cannot say) —
  // built from G on the first Deconvnet walk after an encode (cnn_kernels.h pool_pos_gate_kernel); allocated by that walk
  DevBuf Dg;
  long dg_epoch = -1;
  // 2:4-sparse consumer of the pooled boundary behind this layer (conv_sparse.h; layers with cin % 256 == 0 whose output is pooled:
  // VGG16 block3_conv3, block4_conv3): the four class arrangements of w+ and, per encode, the index planes of the pool's positions
  DevBuf w_sp, idxp;
  long idx_epoch = -1;
  bool sparse_ok() const { return pool_after && conv_sparse_supports(cin, cout, H / 2, W / 2) && !(H & 1) && !(W & 1); }
  DevBuf raw_w_dev, raw_b_dev;       // the arrays as set (HWIO / (cout,)): the fine-tune step's master weights start here
  DevBuf fnorm;    // {largest absolute row sum of w, max|b|}: bound behind the scale of the pairs this layer emits (fwd_scale_kernel)
  bool norm_dirty = true;
  DevBuf Akeep;    // fine-tune step only: a_l of the layers whose output is the next conv's input (no pool after); the
                   // LRP path turns that storage into the gate in place
  size_t act_elems() const { return (size_t)H * W * cout; }
};

struct Encoder {
  int img_h = 0, img_w = 0, max_images = 0, max_tokens = 0;
  int top_h = 0, top_w = 0, top_c = 0;
  std::vector<ConvLayer> layers;
  DevBuf images;           // [max_images][H][W][3]   (x of the image layer, needed by img_stencil_kernel)
  DevBuf a1;               // im2col of the image layer [max_images*H*W][64]
  DevBuf bufX, bufA, bufZ; // forward ping-pong (per call, all images)
  DevBuf bufXs;            // split8 copy of the current conv input (mixed-precision forward)
  DevBuf bufXl;            // its [h | l] companion (three-way split forward product)
  DevBuf feat;             // [max_images][top_h*top_w][top_c]  top activations (== CNN features)
  DevBuf ztop;             // [max_images][top...] Z+ of the top layer
  DevBuf s0, s1;           // reverse-walk ping-pong [max_tokens][biggest layer]
  int encoded = 0;         // images currently cached
  bool features_only = false;
  int prec = PREC_BF16X3;  // arithmetic of the per-token reverse walk (lrp_set_precision); falls back to fp32 for widths % 8 != 0
  const int* row2img_host = nullptr;   // host copy of the NEXT explain call's token -> image map (one-shot; lets the launcher
                                       // order the tiles so that an image's gates are fetched once, conv_args.h TileOrder)
  bool walk_f16 = false;   // LRP_PREC_F16X2 (opt-in): the LRP reverse walk on fp16 pairs, 2 MFMAs per product below the top block.
  // Which layers take the two-MFMA form in that mode (reverse launch through layer li AND its forward denominators Z+_li: the
  // two always go together).  -1 = the built-in rule (every layer up to the last pool whose sums have >= 576 products);
  // otherwise bit li (lrp_set_fast_layers: a per-model choice, e.g. from calibration.py's measured per-layer error).
  int64_t t2_mask_user = -1;
  bool two_term(int li) const {
    if (li <= 0 || li >= (int)layers.size()) return false;
    if (t2_mask_user >= 0) return ((t2_mask_user >> li) & 1) != 0;
    int last_pool = -1;
    for (size_t q = 0; q < layers.size(); ++q)
      if (layers[q].pool_after) last_pool = (int)q;
    return li <= last_pool && 9 * layers[li].cout >= 576 && 9 * layers[li].cin >= 576;   // (narrow test nets: too few products to average over)
  }
                           // Its parity depends on the weight statistics (one fp16 per weight: worst case 2^-12 per product, above the
                           // 1e-4 bar; tests/test_gpu_stress_parity.py), so the default is the three-MFMA split-bf16 walk.
  DevBuf sp_scp;                      // sparse consumers: S_c of the call as chunk-major pairs (conv_sparse.h)
  DevBuf act_max, act_unscale;        // fp16-pair forward: per layer ACT_MAX_SLOTS maxima of its output / 2^-k of its input
  DevBuf out_scale;                   // ... and 2^k of the pairs a layer emits for its consumer (no split pass in between)
  static bool fwd_emit() { return sw().fwd_emit != 0; }   // LRP_FWD_EMIT=0: absmax / split / gate passes between the convs (forward_pairs_split)
  DevBuf tok_exp, tok_max, tok_fac;   // its per-token scale exponents / measured maxima [layers + 1][max_tokens], factors [max_tokens]
  Profiler prof;                      // one record per layer of a reverse walk (common.h)
  // Overlapped encode (mixed-precision mode): the caller's stream runs only the activation chain a_1..a_top (what
  // the decoder needs); the denominators Z+_l and the gates G_l — needed by explain() only — run on `side` behind
  // it, i.e. concurrently with the latency-bound decoder replay the caller enqueues next.
  hipStream_t side = nullptr;
  hipEvent_t ev_fwd = nullptr, ev_gates = nullptr;
  bool gates_pending = false;

  ~Encoder() {
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
    if (ev_fwd) (void)hipEventDestroy(ev_fwd);
    if (ev_gates) (void)hipEventDestroy(ev_gates);
  }
  static bool img_fused() { return sw().img_fused != 0; }   // LRP_IMG_FUSED=0: separate T GEMM + img_stencil_kernel
  bool fwd_fast = false;                                     // LRP_PREC_BF16X3_FAST: the activation convs run split-bf16 too (encoder_forward.h)
  static bool fwd_il() { return sw().fwd_il != 0; }          // LRP_FWD_IL=0: stacked instead of interleaved weight rows (encoder_forward.h)
  // the image layer's fp32 dual GEMM with interleaved rows: gate, pairs and maximum leave its epilogue (no gate / absmax / split pass)
  static bool image_layer_interleaved(const ConvLayer& L) { return fwd_il() && !(L.cout & 31) && conv_npad(2 * L.cout) == 2 * L.cout && !L.pool_after; }
  static bool dual_interleaved(const ConvLayer& L) { return fwd_il() && !(L.cout & 31) && conv_npad(2 * L.cout) == 2 * L.cout; }
  int64_t* ws_total = nullptr;   // the handle's workspace counter (what a walk allocates on its first use is counted too)
  int init(const lrp_config& c, int64_t* total) {
    ws_total = total;
    img_h = c.img_h; img_w = c.img_w; max_images = c.max_images; max_tokens = c.max_tokens;
    if (c.n_conv < 1 || c.n_conv > LRP_MAX_CONV) return fail(LRP_ERR_INVALID, "n_conv=%d out of range", c.n_conv);
    if (c.conv_cin[0] != 3) return fail(LRP_ERR_UNSUPPORTED, "first conv must read a 3-channel image");
    int H = img_h, W = img_w;
    size_t max_act = 0;
    layers.resize(c.n_conv);
    rules.layer.resize(c.n_conv); dl.layer.resize(c.n_conv); pat.layer.resize(c.n_conv);
    for (int i = 0; i < c.n_conv; ++i) {
      ConvLayer& L = layers[i];
      L.name = c.conv_name[i];
      L.cin = c.conv_cin[i]; L.cout = c.conv_cout[i]; L.H = H; L.W = W;
      L.pool_after = c.conv_pool_after[i] != 0;
      if (i > 0 && L.cin != layers[i - 1].cout) return fail(LRP_ERR_INVALID, "conv %d: cin != previous cout", i);
      if (L.cout % 4 != 0) return fail(LRP_ERR_UNSUPPORTED, "conv %d: cout must be a multiple of 4", i);
      if (i == c.n_conv - 1 && L.pool_after) return fail(LRP_ERR_UNSUPPORTED, "encoder must end with a conv layer");
      if (L.act_elems() > max_act) max_act = L.act_elems();
      if (L.pool_after) {
        if ((H & 1) || (W & 1)) return fail(LRP_ERR_UNSUPPORTED, "odd resolution before a 2x2 pool");
        H >>= 1; W >>= 1;
      }
    }
    const ConvLayer& T = layers.back();
    top_h = T.H; top_w = T.W; top_c = T.cout;
    if (top_h * top_w != c.L || top_c != c.D)
      return fail(LRP_ERR_INVALID, "encoder output (%d x %d x %d) does not match L=%d, D=%d", top_h, top_w, top_c, c.L, c.D);
    const size_t B = (size_t)max_images, NT = (size_t)max_tokens;
    const size_t max_tok_act = std::max(max_act, (size_t)img_h * img_w * IMG_T_COLS);   // T of the image layer
    LRP_TRY(images.alloc(B * img_h * img_w * 3 * sizeof(float), total));
    LRP_TRY(a1.alloc(B * img_h * img_w * 64 * sizeof(float), total));
    LRP_TRY(bufX.alloc(B * max_act * sizeof(float), total));
    LRP_TRY(bufA.alloc(B * max_act * sizeof(float), total));
    LRP_TRY(bufZ.alloc(B * max_act * sizeof(float), total));
    LRP_TRY(bufXs.alloc(B * max_act * sizeof(float), total));
    LRP_TRY(bufXl.alloc(B * max_act * sizeof(float), total));
    LRP_TRY(feat.alloc(B * T.act_elems() * sizeof(float), total));
    LRP_TRY(ztop.alloc(B * T.act_elems() * sizeof(float), total));
    LRP_TRY(s0.alloc(NT * max_tok_act * sizeof(float), total));
    LRP_TRY(s1.alloc(NT * max_tok_act * sizeof(float), total));
    for (size_t i = 0; i + 1 < layers.size(); ++i) LRP_TRY(layers[i].G.alloc(B * layers[i].act_elems() * sizeof(float), total));
    for (size_t i = 0; i + 1 < layers.size(); ++i) {
      ConvLayer& Lc = layers[i];                         // compact gate: where the layer's reverse launch can read it at some token count
      if (Lc.pool_after && conv_compact_shape(Lc.cin, Lc.cout, Lc.H, Lc.W)) {
        LRP_TRY(Lc.Gc.alloc(B * Lc.act_elems() / 4 * sizeof(float), total));
        LRP_TRY(Lc.Gpos.alloc(B * Lc.act_elems() / 4, total));
      }
    }
    for (size_t i = 0; i + 1 < layers.size(); ++i)
      if (layers[i].pool_after) LRP_TRY(layers[i].P.alloc(B * layers[i].act_elems() / 4 * sizeof(float), total));
    {  // sparse consumers: index planes per image, one chunk-major copy of S_c per call (the largest of them)
      size_t mx = 0;
      for (size_t i = 1; i + 1 < layers.size(); ++i) {
        ConvLayer& Lc = layers[i];
        if (!Lc.sparse_ok() || !Lc.Gpos.p || layers[i - 1].pool_after) continue;
        LRP_TRY(Lc.idxp.alloc(conv_sparse_index_words((int)B, Lc.H / 2, Lc.W / 2, Lc.cout) * sizeof(unsigned), total));
        mx = std::max(mx, NT * Lc.act_elems() / 4);
      }
      if (mx) LRP_TRY(sp_scp.alloc(mx * sizeof(float), total));
    }
    {
      // lowest priority: the side work is throughput work that should only fill what the caller's stream leaves idle
      int lo = 0, hi = 0;
      LRP_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      LRP_HIP_CHECK(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, lo));
    }
    LRP_HIP_CHECK(hipEventCreateWithFlags(&ev_fwd, hipEventDisableTiming));
    LRP_HIP_CHECK(hipEventCreateWithFlags(&ev_gates, hipEventDisableTiming));
    // scale records of the fp16-pair forward, per layer AND image (the emitting forward scales every image by its own
    // maxima; +1 level: the images themselves)
    LRP_TRY(act_max.alloc((layers.size() + 1) * B * ACT_MAX_SLOTS * sizeof(unsigned), total));
    LRP_TRY(act_unscale.alloc((layers.size() + 1) * B * sizeof(float), total));
    LRP_TRY(out_scale.alloc((layers.size() + 1) * B * sizeof(float), total));
    for (ConvLayer& L : layers) LRP_TRY(L.fnorm.alloc(2 * sizeof(float), total));
    return LRP_OK;
  }

  size_t max_act_elems() const {
    size_t m = 0;
    for (const ConvLayer& L : layers) m = std::max(m, L.act_elems());
    return m;
  }

  // ---- the analyzers' state (encoder_state.h) and the few questions the hot path asks about it ----
  RuleTableState rules;
  DeepLiftState dl;
  TraceState tr;
  PatternState pat;
  bool table_on() const { return rules.on(); }
  // epsilon kinds are exact-fp32 only (their gate a / (a + eps) is a step in a for small eps: a ReLU decision the fp16-pair forward
  // takes differently moves the map by O(1)); fp16 pairs have no table walk at all
  bool table_runs() const { return !walk_f16 && (!rules.has_eps() || prec == PREC_FP32); }
  bool rule_split() const {                              // the table's arithmetic follows the handle's mode (as walk_mode's split)
    return prec == PREC_BF16X3 && std::none_of(layers.begin(), layers.end(), [](const ConvLayer& L) { return (L.cout & 7) != 0; });
  }
  bool table_split() const { return rule_split() && !rules.has_eps(); }
  const ConvRule& rule_at(int li) const { static const ConvRule def; return table_on() ? rules.table[li] : def; }   // (no table: the default rule)
  const float* table_gate(int li) const { return rules.table[li].own_gate() ? rules.layer[li].Gt.as<float>() : layers[li].G.as<float>(); }
  bool dl_active() const { return dl.mode != 0 && prec == PREC_FP32; }
  // layer li's weights changed: the table's matrices are repacked by the next encode under a table, A * w by the next pattern walk,
  // and the reference's activations belong to the old weights
  void analyzers_stale(int li) { rules.layer[li].packed = false; pat.layer[li].packed = false; dl.ref_stale = true; }

  // Fine-tune step: the weight gradient of layer l needs a_{l-1}; keep what the LRP caches drop.
  // Five users, each for itself, so that none can switch another's activations off: the fine-tune step (for the life of the handle
  // once lrp_train_begin ran), a rule table (while it is set), a DeepLIFT reference (while it is set and the handle is in
  // LRP_PREC_FP32: its walk runs nowhere else, and the other modes' forwards keep their fused forms), the layer trace (while it is
  // on) and a pattern fit (pattern_fit_begin .. pattern_fit_end).  encode() decides keep_acts from the five.
  bool keep_acts = false, keep_for_train = false;
  bool acts_wanted() const { return keep_for_train || table_on() || dl_active() || tr.on || pat.type >= 0; }
  int alloc_keep_acts(int64_t* total) {
    for (size_t li = 0; li + 1 < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      if (!L.pool_after && !L.Akeep.p) LRP_TRY(L.Akeep.alloc((size_t)max_images * L.act_elems() * sizeof(float), total));   // (kept across a rule round trip)
    }
    return LRP_OK;
  }
  int enable_keep_acts(int64_t* total) {                 // the fine-tune step
    LRP_TRY(alloc_keep_acts(total));
    keep_acts = keep_for_train = true;
    return LRP_OK;
  }
  // input of conv li as the last encode left it (li >= 1; the image itself for li = 0)
  const float* layer_input(int li) const {
    if (li == 0) return images.as<float>();
    const ConvLayer& P = layers[li - 1];
    return P.pool_after ? P.P.as<float>() : P.Akeep.as<float>();
  }

  int find_layer(const std::string& nm) const {
    for (size_t i = 0; i < layers.size(); ++i)
      if (layers[i].name == nm) return (int)i;
    return -1;
  }

  // ---- the device packers (encoder_weights.h) ----
  DevBuf pack_tmp;                                    // scratch of the device packers (largest forward matrix)
  DevBuf f16_slots;                                    // ACT_MAX_SLOTS maxima while a weight matrix' fp16 copy is made
  int alloc_conv_operands(int li, int64_t* total, hipStream_t st);
  int repack_conv_weight_from_device(int li, const float* w_dev, float* tmp, hipStream_t st);
  int repack_conv_from_device(int li, const float* w_dev, const float* b_dev, float* tmp, hipStream_t st);
  int set_conv_weight_dev(int li, const float* w, hipMemcpyKind kind, int64_t* total, hipStream_t st),
      set_conv_bias_dev(int li, const float* b, hipMemcpyKind kind, int64_t* total, hipStream_t st);

  int check_ready() const {
    for (const ConvLayer& L : layers)
      if (!L.have_w || !L.have_b) return fail(LRP_ERR_STATE, "encoder weights for layer '%s' not set", L.name.c_str());
    return LRP_OK;
  }

  // ---- forward once per image -------------------------------------------------------------
  long encode_epoch = 0;   // bumped by every encode: a layer's compact gate is current iff its gc_epoch equals this
  int encode(const float* images_dev, int B, hipStream_t st) {
    if (B < 1 || B > max_images) return fail(LRP_ERR_INVALID, "B=%d outside [1,%d]", B, max_images);
    LRP_TRY(check_ready());
    keep_acts = acts_wanted();
    if (dl_active() && dl.ref_stale) LRP_TRY(dl_reference_pass(st));
    ++encode_epoch;
    for (ConvLayer& L : layers) L.gfull_epoch = encode_epoch;     // (every path writes the full-resolution gates, except the fused pool: after_pool_gate)
    const size_t img_elems = (size_t)img_h * img_w * 3;
    LRP_TRY(wait_gates(st, true));                     // the previous encode's side work still owns G / bufZ / bufXs
    LRP_HIP_CHECK(hipMemsetAsync(act_max.p, 0, act_max.bytes, st));
    LRP_HIP_CHECK(hipMemcpyAsync(images.p, images_dev, B * img_elems * sizeof(float), hipMemcpyDeviceToDevice, st));
    // emitting needs every layer on the interleaved dual matrix (the pairs and the gate leave one epilogue: decided when the
    // weights were packed)
    std::vector<int> widths;
    bool emit_ready = fwd_emit() && !(img_elems & 3);
    for (const ConvLayer& L : layers) {
      widths.push_back(L.cout);
      if (!L.w_fwd_il.p) emit_ready = false;
    }
    const FwdPlan fp = forward_mode(prec == PREC_BF16X3, fwd_fast, widths.data(), widths.size(), layers[0].pool_after, emit_ready);
    LRP_TRY(fp.mode == FWD_EXACT ? forward_exact(B, st) : fp.mode == FWD_FAST ? forward_fast(B, st)
            : fp.emit ? forward_pairs_emit(B, st) : forward_pairs_split(B, st));
    encoded = B;
    if (table_on() && table_runs()) {
      const int rc = table_pass(B, st);
      if (rc != LRP_OK) { encoded = 0; return rc; }
    }
    if (dl_active()) {
      const int rc = dl_pass(B, st);
      if (rc != LRP_OK) { encoded = 0; return rc; }
    }
    features_only = false;
    return LRP_OK;
  }

  // ---- launch helpers of the forwards ----
  static int launched() { LRP_HIP_CHECK(hipGetLastError()); return LRP_OK; }
  // geometry of the 3x3 conv through layer L over NB images (or relevance maps) reading `in`, C channels wide
  static ConvArgs conv3x3_args(const ConvLayer& L, int NB, const float* in, int C) {
    ConvArgs ca{};
    ca.in = in; ca.NB = NB; ca.H = L.H; ca.W = L.W; ca.Cin = C; ca.CinP = conv_cinp(C); ca.taps = 9;
    return ca;
  }
  // ---- the four forwards and their launch helpers (encoder_forward.h) ----
  // Scale records of layer / level `lev` of the fp16-pair forwards: ACT_MAX_SLOTS maxima of its output, 2^-k of its input, 2^k of
  // the pairs it emits.  `per` of each per layer: one for the whole batch, or — emitting — one per image, so that an image's result
  // does not depend on the rest of its batch.
  struct ScaleRecs {
    unsigned* max; float *unscale, *oscale; size_t per;
    unsigned* slots_of(size_t lev) const { return max + lev * per * ACT_MAX_SLOTS; }
    float* unscale_of(size_t li) const { return unscale + li * per; }
    float* oscale_of(size_t li) const { return oscale + li * per; }
  };
  ScaleRecs scale_recs(size_t per) const { return {act_max.as<unsigned>(), act_unscale.as<float>(), out_scale.as<float>(), per}; }
  static ConvArgs fwd_conv_args(const ConvLayer& L, int B, const float* in);
  int im2col_gemm_args(int B, hipStream_t st, ConvArgs& ca);
  int gate_pass(ConvLayer& L, int B, const float* a, const float* z, hipStream_t st), maxpool_pass(ConvLayer& L, int B, const float* a, hipStream_t st);
  int pool_gate_pass(ConvLayer& L, int B, const float* a, const float* z, float* pooled, hipStream_t st), split_copy(const float* src, size_t n8, hipStream_t st);
  const float* parked_act(const ConvLayer& L) const;
  float* act_out(ConvLayer& L, bool top);
  int dual_fp32_layer(size_t li, int B, hipStream_t st, float*& x, float*& a, float* z);
  ConvArgs dual_pairs_args(size_t li, int B, const float* pin, const ScaleRecs& r, bool per_img);
  void fuse_gate(ConvLayer& L, ConvArgs& cd, const float* x_in);
  int fwd_terms(size_t li, const ConvArgs& cd) const;
  int after_pool_gate(size_t li, int B, hipStream_t st, bool full_written);
  int image_layer_emit(int B, hipStream_t st, const ScaleRecs& r, float* pairs_out);
  int forward_exact(int B, hipStream_t st), forward_fast(int B, hipStream_t st), forward_pairs_split(int B, hipStream_t st),
      forward_pairs_emit(int B, hipStream_t st);

  // ---- reverse walk, n relevance maps at once ---------------------------------------------
  // The walks that read a pooled layer's gate at full resolution (EPI_MUL_UP2: the gradient baselines, the fp32 and fast modes,
  // pooled boundaries without a pairs consumer, LRP_UP2_COMPACT=0) after an encode whose fused pool epilogue left the compact form only
  int full_gate(int li, hipStream_t st) {
    ConvLayer& L = layers[li];
    if (!L.pool_after || L.gfull_epoch == encode_epoch) return LRP_OK;
    if (!L.Gc.p || L.gc_epoch != encode_epoch) return fail(LRP_ERR_STATE, "no pool gate of layer %d for this encode", li);
    const size_t n8 = (size_t)encoded * (L.H / 2) * (L.W / 2) * (L.cout / 8);
    hipLaunchKernelGGL(pool_gate_expand_kernel, dim3(stream_grid(n8)), dim3(256), 0, st, L.Gc.as<float>(), L.Gpos.as<unsigned char>(),
                       L.G.as<float>(), encoded, L.H, L.W, L.cout);
    LRP_HIP_CHECK(hipGetLastError());
    L.gfull_epoch = encode_epoch;
    return LRP_OK;
  }

  // Deconvnet: the 0/1 position gate of pooled layer li (ConvLayer::Dg) for this encode
  int position_gate(int li, hipStream_t st) {
    ConvLayer& L = layers[li];
    if (L.dg_epoch == encode_epoch) return LRP_OK;
    LRP_TRY(full_gate(li, st));
    if (!L.Dg.p) LRP_TRY(L.Dg.alloc((size_t)max_images * L.act_elems() * sizeof(float), ws_total));
    const size_t n4 = (size_t)encoded * (L.H / 2) * (L.W / 2) * (L.cout / 4);
    hipLaunchKernelGGL(pool_pos_gate_kernel, dim3(stream_grid(n4)), dim3(256), 0, st, L.G.as<float>(), L.Dg.as<float>(), encoded, L.H,
                       L.W, L.cout);
    LRP_HIP_CHECK(hipGetLastError());
    L.dg_epoch = encode_epoch;
    return LRP_OK;
  }

  // What one explain call runs, decided once at its top (walk_mode)
  struct WalkMode {
    int n = 0, walk = 0, run_prec = PREC_FP32;
    bool hook = false;                                 // fine-tune step: the layer hook is called, the image layer skipped
    bool split = false, hook_split = false, f16 = false, fold_on = false;
    // the default walk: what the compact pool interface, the sparse consumers and the folded image layer belong to
    bool lrp_split() const { return split && !f16 && walk == 0 && !hook; }
  };
  WalkMode walk_mode(int n, int walk, bool hook) const {
    WalkMode m;
    m.n = n; m.walk = walk; m.hook = hook;
    m.split = prec == PREC_BF16X3 && walk == 0;        // the LRP walk on split-bf16 operands
    // Fine-tune step (hook, walk = 1) in the default arithmetic: the backward-data convs run split-bf16 too —
    // bf16 operands (hi + lo), three MFMAs per product, fp32 accumulate; the hook still sees plain fp32 dZ (the weight
    // gradient reads it), so every layer's dZ is written fp32 and re-split by one streaming pass in front of its conv.
    m.hook_split = prec == PREC_BF16X3 && walk == 1 && hook;
    for (const ConvLayer& L : layers)
      if (L.cout & 7) m.split = m.hook_split = false;   // split8 groups need widths % 8 == 0: exact fp32 otherwise
    for (size_t li = 1; li < layers.size(); ++li)
      if (!layers[li].w_bwd_full_s.p) m.hook_split = false;
    // LRP_PREC_F16X2: fp16 pairs for S, one fp16 per weight, per-token power-of-two scales (conv_args.h PREC_F16X2);
    // needs the fused image layer (the chain's scale is undone in its epilogue)
    m.f16 = m.split && walk_f16 && img_fused();
    m.run_prec = m.f16 ? PREC_F16X2 : (m.split || m.hook_split) ? PREC_BF16X3 : PREC_FP32;
    // Image layer folded into the epilogue of the layer above it (ConvArgs::img_part): S_1 — 4.1 GB written, 4.5 GB read at
    // the bench configuration — never goes to memory; per tile 160 positions x 6 partial sums do, and a streaming pass
    // adds them up in a fixed order [MI355X, same box: block1_conv2 4.25 -> 4.57 ms (it now also runs the tap GEMM and the
    // in-tile stencil), image layer 1.29 -> 0.18 ms, walk 26.1-26.3 -> 25.3 ms; heat-maps unchanged to fp32 round-off,
    // batch invariance bit-exact].  LRP_IMG_FOLD=0 disables.
    m.fold_on = sw().img_fold != 0 && m.lrp_split() && img_fused() && layers.size() > 1 && !layers[0].pool_after &&
                layers[1].cin == 64 && layers[0].w_bwd_s.p != nullptr;
    return m;
  }
  // conv_plan's answer for the dense launch through layer lc (lc >= 1) of this walk: with the folded image layer on it where
  // that is wanted, and reading the compact pool interface or not
  ConvPlan walk_plan(const WalkMode& m, int lc, bool up2) const {
    const ConvLayer& Lc = layers[lc];
    ConvAsk q;
    q.epi = layers[lc - 1].pool_after ? EPI_MUL_UP2 : EPI_MUL; q.prec = m.run_prec;      // (asked for the split-bf16 walk only)
    q.NB = m.n; q.H = Lc.H; q.W = Lc.W; q.N = Lc.cin; q.Cin = Lc.cout; q.taps = 9;
    q.frag = m.split && m.walk == 0 && Lc.w_bwd_frag.p != nullptr;
    q.up2_src = up2; q.img_part = lc == 1 && m.fold_on;
    return conv_plan(q);
  }
  // Does layer lc's launch run on the 2:4-sparse matrix cores (conv_sparse.h)?  Decided by the layer's shape, the precision
  // and what this encode left — never by the token or image count: sparse and dense sum in different orders, and a picture's
  // heat-map must not depend on the batch it is explained in.  LRP_SPARSE_POOL=0 disables.
  bool sparse_consumer(const WalkMode& m, int lc) const {
    if (lc < 1) return false;
    const ConvLayer& Lc = layers[lc];
    return sw().sparse_pool && Lc.w_sp.p && Lc.idxp.p && Lc.idx_epoch == encode_epoch && !layers[lc - 1].pool_after && m.lrp_split() &&
           sp_scp.p != nullptr;
  }
  // Compact pool interface (conv_args.h ConvArgs::up2_src): the producer of a pooled boundary (layer li, its consumer li - 1)
  // multiplies with the consumer's COMPACT gate (one value per window and channel, at the producer's resolution) and writes
  // S_c as bf16 pairs at POOLED resolution; the consumer builds its resident image from the pairs and the position bytes:
  // the 4x-expanded, 75 %-zero tensor is neither written nor read.  Only two dense consumers can: the folded weights-in-registers
  // launch (VGG16 block1_conv2: per-token tiles, its window loader) and the pipelined halo kernels; conv_plan says whether the
  // consumer's launch is one of them, and both need a compact gate from this encode.  Every other pooled boundary takes
  // EPI_MUL_UP2 (the expanded tensor; same fp32 product, same pairs).  LRP_UP2_COMPACT=0 disables.
  // Does the launch of layer li write those pairs for its consumer li - 1?  A sparse consumer reads nothing else, so its
  // producer writes them whatever LRP_UP2_COMPACT / LRP_UP2_PW say and whatever tile the producer takes (a plain EPI_MUL
  // epilogue with the compact gate); those two switches govern the boundaries whose consumer is dense.
  bool writes_pairs(const WalkMode& m, int li) const {
    const ConvLayer& P = layers[li - 1];
    if (!P.pool_after || !m.lrp_split() || li < 2 || (P.cout & 7) || !P.Gc.p || P.gc_epoch != encode_epoch) return false;
    if (sparse_consumer(m, li - 1)) return true;
    return sw().up2_compact != 0 && walk_plan(m, li - 1, true).ok;
  }
  int* lev_exp(int lev) const { return tok_exp.as<int>() + (size_t)lev * max_tokens; }          // PREC_F16X2: per-token scale
  unsigned* lev_max(int lev) const { return tok_max.as<unsigned>() + (size_t)lev * max_tokens; }   // exponents / maxima of level lev
  // algorithmic flops of the reverse launch through layer li (the image layer: 6 sums per pixel and tap)
  double layer_flop(int n, int li) const { return 2.0 * (double)n * layers[li].H * layers[li].W * 9.0 * layers[li].cout * (li == 0 ? 6 : layers[li].cin); }

  // top of the chain: S_top = R / safe(Z+_top) in the form the walk's first launch reads (gradient walks: the head's gradient
  // through the top ReLU)
  int top_relevance(const WalkMode& m, const int* row2img_dev, const float* R_feat_dev, float* S, hipStream_t st) {
    const ConvLayer& T = layers.back();
    const size_t per4 = T.act_elems() / 4, per8 = T.act_elems() / 8;
    const int n = m.n;
    if (m.walk != 0) {
      hipLaunchKernelGGL(grad_top_kernel, dim3(stream_grid((size_t)n * per4)), dim3(256), 0, st,
                         reinterpret_cast<const f32x4*>(R_feat_dev), feat.as<f32x4>(), row2img_dev,
                         reinterpret_cast<f32x4*>(S), n, per4, m.walk == 4 ? 2 : m.walk == 3 ? 1 : 0);
    } else if (m.f16) {
      const int top = (int)layers.size() - 1;
      hipLaunchKernelGGL(top_divide_f16_kernel, dim3(n), dim3(256), 0, st, R_feat_dev, ztop.as<float>(), row2img_dev, S,
                         per8, lev_exp(top), lev_max(top));
    } else if (m.split) {
      hipLaunchKernelGGL(top_divide_split_kernel, dim3(stream_grid((size_t)n * per8)), dim3(256), 0, st, R_feat_dev,
                         ztop.as<float>(), row2img_dev, S, n, per8);
    } else {
      hipLaunchKernelGGL(top_divide_kernel, dim3(stream_grid((size_t)n * per4)), dim3(256), 0, st,
                         reinterpret_cast<const f32x4*>(R_feat_dev), ztop.as<f32x4>(), row2img_dev,
                         reinterpret_cast<f32x4*>(S), n, per4);
    }
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }
  // the pooled boundary below layer li on the 2:4-sparse matrix cores (conv_sparse.h): S_c re-laid chunk-major, then one launch per class
  int sparse_boundary(int li, int n, const int* row2img_dev, const float* S, float* out, hipStream_t st) {
    const ConvLayer& L = layers[li];
    const int Hp = L.H / 2, Wp = L.W / 2;
    const size_t n_sets = (size_t)n * Hp * Wp * (L.cout / 8);
    prof.begin(st);
    hipLaunchKernelGGL(conv_sparse_relayout_kernel, dim3(stream_grid(n_sets)), dim3(256), 0, st, S, sp_scp.as<float>(), n_sets, Hp * Wp, L.cout);
    LRP_HIP_CHECK(hipGetLastError());
    SparseArgs sa{};
    sa.sc = sp_scp.as<float>(); sa.idxp = L.idxp.as<unsigned>(); sa.wsp = L.w_sp.as<float>(); sa.gate = layers[li - 1].G.as<float>(); sa.out = out;
    sa.row2img = row2img_dev; sa.NB = n; sa.Hp = Hp; sa.Wp = Wp; sa.C = L.cout; sa.N = L.cin;
    LRP_HIP_CHECK(conv_sparse_launch(sa, st));
    prof.end(st, layer_flop(n, li));
    return LRP_OK;
  }
  // the folded image layer's second half: the tiles' partial sums -> R_img (its algorithmic flops are booked on this record)
  int fold_image_sum(int n, const ConvPlan& fold, const float* part, const int* row2img_dev, float* R_img_dev, hipStream_t st) {
    const ConvLayer& L0 = layers[0];
    prof.begin(st);
    hipLaunchKernelGGL(img_partial_sum_kernel, dim3(stream_grid((size_t)n * L0.H * L0.W)), dim3(256), 0, st, part, images.as<float>(),
                       row2img_dev, R_img_dev, n, L0.H, L0.W, fold.th, fold.tw, fold.cols_t, 0);
    LRP_HIP_CHECK(hipGetLastError());
    prof.end(st, layer_flop(n, 0));
    return LRP_OK;
  }

  // The image layer's launch of a walk; `ca` holds the input, the matrix and row2img.  T GEMM + 9-tap stencil in one launch (patch
  // tiles, T stays in LDS) into R_img_dev — or, with LRP_IMG_FUSED=0, the 1-tap GEMM over the pixels into T, which
  // image_stencil_tail turns into R_img_dev.  Returns the epilogue.
  int image_layer_args(ConvArgs& ca, int n, float* T, float* R_img_dev, int img_mode, float lo, float hi) const {
    const ConvLayer& L = layers[0];
    ca.taps = 1; ca.N = IMG_T_COLS;
    if (img_fused()) {
      ca.out = R_img_dev; ca.ximg = images.as<float>(); ca.img_mode = img_mode; ca.img_lo = lo; ca.img_hi = hi;
      return EPI_IMG_STENCIL;
    }
    ca.NB = n * L.H * L.W; ca.H = 1; ca.W = 1; ca.out = T;
    return EPI_STORE;
  }
  // LRP_IMG_FUSED=0: T (n, H, W, 54) -> R_img_dev, the 9-tap shift-and-add and the selection of x+ / x- (or what img_mode says)
  int image_stencil_tail(int n, const float* T, const int* row2img_dev, float* R_img_dev, int img_mode, float lo, float hi, hipStream_t st) {
    if (img_fused()) return LRP_OK;
    const ConvLayer& L0 = layers[0];
    hipLaunchKernelGGL(img_stencil_kernel, dim3(stream_grid((size_t)n * L0.H * L0.W)), dim3(256), 0, st, T, images.as<float>(), row2img_dev,
                       R_img_dev, n, L0.H, L0.W, img_mode, lo, hi);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }

  // ---- steps the walks share: an analyzer walk reads as head, loop body, tail, with only its own streaming kernel spelled out ----
  // What a walk's checks start and end with; its mode checks stand between them — mode before state: a refusal says what to change
  // first.  `what` ends the sentence, `also` is the walk's own condition on that encode.
  int tokens_ok(int n) const { return n < 1 || n > max_tokens ? fail(LRP_ERR_INVALID, "n=%d outside [1,%d]", n, max_tokens) : LRP_OK; }
  int encoded_ok(const char* what, bool also = true) const {
    return encoded < 1 || features_only || !also ? fail(LRP_ERR_STATE, "lrp_encode_images must run %s", what) : LRP_OK;
  }
  // The overlapped forwards leave gates / Z_top to the side stream: whoever reads or replaces them on `st` waits here first — every
  // walk (explain_deeplift included, although the exact-fp32 encode it insists on never leaves side work behind), and with `retire`
  // the calls that every later call is ordered behind (encode, its passes, a weight upload).
  int wait_gates(hipStream_t st, bool retire = false) {
    if (gates_pending) LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_gates, 0));
    if (retire) gates_pending = false;
    return LRP_OK;
  }
  // a workspace buffer that appears, or grows, with the first call that needs it at that size (the old size leaves the handle's
  // count); zero: 0 as it comes | 1 cleared now | 2 cleared in stream order on st (padding rows / columns stay zero)
  static int grow(DevBuf& d, size_t bytes, int64_t* total, int zero = 0, hipStream_t st = nullptr) {
    if (d.p && d.bytes >= bytes) return LRP_OK;
    if (d.p && total) *total -= (int64_t)d.bytes;
    LRP_TRY(d.alloc(bytes, total));
    if (zero) LRP_HIP_CHECK(zero == 1 ? hipMemset(d.p, 0, d.bytes) : hipMemsetAsync(d.p, 0, d.bytes, st));
    return LRP_OK;
  }
  // the ping-pong of a walk's chains: the default walk's, or the two-chain pair of the table that brought it
  void chain_buffers(bool two, float*& S, float*& Snext) const { S = (two ? rules.s0ab : s0).as<float>(); Snext = (two ? rules.s1ab : s1).as<float>(); }
  // one conv of a walk as one profiler record
  int timed_conv(int epi, const ConvArgs& ca, hipStream_t st, int run_prec, double flop, int terms = 7) {
    prof.begin(st);
    LRP_HIP_CHECK(conv_launch(epi, ca, st, run_prec, terms));
    prof.end(st, flop);
    return LRP_OK;
  }
  // epilogue of the launch through layer li >= 1: a gate read through the pool below it, or a plain product
  int mul_epi(int li, const ConvArgs& ca) const { return !ca.gate_none && layers[li - 1].pool_after ? EPI_MUL_UP2 : EPI_MUL; }
  // Every launch of a walk is one conv_plan answers: asked before the first one runs, layers `first` up or down to (not including)
  // `end`.  args_of(li) builds layer li's launch as the walk will (image_layer_args shapes the image layer's), refuse(li) refuses.
  template <class Args, class Refuse>
  int plan_or_refuse(int first, int end, int rows, int run_prec, Args&& args_of, Refuse&& refuse) const {
    for (int li = first, d = end < first ? -1 : 1; li != end; li += d) {
      ConvArgs ca = args_of(li);
      const int epi = li == 0 ? image_layer_args(ca, rows, nullptr, nullptr, 0, 0.f, 0.f) : mul_epi(li, ca);
      if (!conv_plan(conv_ask(epi, run_prec, 7, false, ca)).ok) return refuse(li);
    }
    return LRP_OK;
  }
  // The image layer of an analyzer walk: `ca` holds the input, the matrix and row2img; its launch over `rows` maps as one profiler
  // record, then image_stencil_tail.  T: where LRP_IMG_FUSED=0 parks the tap GEMM's result.
  int image_layer_step(ConvArgs ca, int rows, int run_prec, double flop, float* T, float* R, int img_mode, float lo, float hi, hipStream_t st) {
    const int epi = image_layer_args(ca, rows, T, R, img_mode, lo, hi);
    LRP_TRY(timed_conv(epi, ca, st, run_prec, flop));
    return image_stencil_tail(rows, T, ca.row2img, R, img_mode, lo, hi, st);
  }

  // ---- rule table (encoder_rules.h) ----
  // the backward matrix layer li walks on under its rule: the default walk's, or the table's own
  const float* rule_matrix(int li, bool split) const {
    if (rule_at(li).on_default_matrix()) return (split ? layers[li].w_bwd_s : layers[li].w_bwd).as<float>();
    return (split ? rules.layer[li].w_bwd_t_s : rules.layer[li].w_bwd_t).as<float>();
  }
  void clear_table();
  int set_table(const std::vector<ConvRule>& t, int64_t* total);
  int pack_table_layer(int li, const float* w_dev, hipStream_t st), table_pass(int B, hipStream_t st);
  int rule_head(const ConvRule& r, bool split, int n, const int* row2img_dev, const float* R_feat_dev, float* S, hipStream_t st);
  int explain_table(int n, const int* row2img_dev, const float* R_feat_dev, float* R_img_dev, hipStream_t st);
  // ---- DeepLIFT (encoder_deeplift.h) ----
  int set_deeplift_reference(const float* ref_host, float ref_scalar, int mode, int64_t* total);
  int dl_reference_pass(hipStream_t st), dl_pass(int B, hipStream_t st), dl_check(int n) const;
  static int dl_combine(bool two, bool pool, const float* c, const float* x, const float* xr, const float* dn, const int* r2i, float* out, int n,
                        int H, int W, int C, hipStream_t st);
  static int dl_final(bool two, const float* c, const float* x, const float* xr, const int* r2i, float* out, int n, size_t per, hipStream_t st);
  int explain_deeplift(int n, const int* row2img_dev, const float* head_dev, float* R_img_dev, hipStream_t st);
  // ---- layer trace (encoder_trace.h) ----
  std::vector<TraceTensor> trace_tensors() const;
  int64_t trace_keep_layout(int n, uint64_t mask, std::vector<int64_t>& off) const;
  int trace_index_of_conv(int li) const, trace_check(int n) const;
  int set_layer_trace(bool on, int64_t* total);
  static int trace_chunks(const ConvLayer& L, bool split);
  static int tensor_stats(const float* x, int rows, size_t per_row, double* stats, hipStream_t st);
  static int trace_layer(bool pool, bool split, int k, const TraceLayerArgs& t, int nblk, hipStream_t st);
  int explain_traced(int n, const int* row2img_dev, const float* R_feat_dev, float* R_img_dev, double* stats_dev, float* keep_dev,
                     const std::vector<int64_t>& keep_off, hipStream_t st);
  // ---- PatternNet / PatternAttribution (encoder_pattern.h) ----
  int pattern_mode_check() const, pattern_fit_check() const, pattern_walk_check(int n) const;
  int pattern_fit_begin(int type, int64_t* total);
  int pattern_fit_batch(hipStream_t st), pattern_fit_end(hipStream_t st), pattern_pack(hipStream_t st);
  int pattern_alloc(int li), pattern_set(int li, const float* A_dev, hipStream_t st);
  int pattern_row_div(const float* x, int n, size_t per_row, hipStream_t st);
  int explain_pattern(int n, const int* row2img_dev, const float* head_dev, float* R_img_dev, bool attribution, hipStream_t st);

  // R_feat_dev (n, top_h*top_w, top_c) -> R_img_dev (n, img_h, img_w, 3); row2img_dev: device int[n]
  // walk: 0 = LRP (LRPSequentialPresetA); gradient baselines (gradient_based.py:101-265) on the same caches:
  //   1 = Gradient, 2 = InputTimesGradient, 3 = GuidedBackprop — backward-data convs with the full w, the LRP gate
  //   used as the ReLU/arg-max mask, exact fp32.
  //   4 = Deconvnet (gradient_based.py:180-225): every ReLU clamps what arrives at 0 and passes it on — no forward ReLU decision
  //   is read; the pools route to the forward's arg-max (position_gate), non-pooled boundaries take no gate at all.
  // layer_hook (fine-tune step): called with (li, dZ_li) — the gradient at the pre-activation of conv li, n x H x W x cout —
  // before that layer's backward-data conv is launched; the image layer itself is then skipped (R_img_dev may be null).
  int explain(int n, const int* row2img_dev, const float* R_feat_dev, float* R_img_dev, hipStream_t st, int walk = 0,
              const std::function<int(int, const float*)>* layer_hook = nullptr) {
    const int* r2i_host = row2img_host;
    row2img_host = nullptr;                              // one-shot
    LRP_TRY(tokens_ok(n));
    if (walk < 0 || walk > 4) return fail(LRP_ERR_INVALID, "unknown walk %d", walk);
    LRP_TRY(encoded_ok("before the CNN explain"));
    LRP_TRY(wait_gates(st));
    // (the gradient walks and the fine-tune step ignore the rule)
    if (table_on() && walk == 0 && !layer_hook) return explain_table(n, row2img_dev, R_feat_dev, R_img_dev, st);
    const WalkMode m = walk_mode(n, walk, layer_hook != nullptr);
    const int img_mode = walk == 0 ? 0 : walk == 2 ? 2 : 1;
    float *S = s0.as<float>(), *Snext = s1.as<float>();
    if (m.f16) {
      const size_t cnt = (layers.size() + 1) * (size_t)max_tokens;
      if (!tok_exp.p) {
        int64_t dummy = 0;
        LRP_TRY(tok_exp.alloc(cnt * sizeof(int), &dummy));
        LRP_TRY(tok_max.alloc(cnt * sizeof(unsigned), &dummy));
        LRP_TRY(tok_fac.alloc((size_t)max_tokens * sizeof(float), &dummy));
      }
      LRP_HIP_CHECK(hipMemsetAsync(tok_max.p, 0, cnt * sizeof(unsigned), st));
    }
    LRP_TRY(top_relevance(m, row2img_dev, R_feat_dev, S, st));
    bool pairs_in = false;                               // S (the current layer's input) is S_c as pairs at pooled resolution
    for (int li = (int)layers.size() - 1; li >= 0; --li) {
      const ConvLayer& L = layers[li];
      if (layer_hook) {
        LRP_TRY((*layer_hook)(li, S));
        if (li == 0) return LRP_OK;
      }
      if (pairs_in && sparse_consumer(m, li)) {
        LRP_TRY(sparse_boundary(li, n, row2img_dev, S, Snext, st));
        pairs_in = false;
        std::swap(S, Snext);
        continue;
      }
      ConvArgs ca = conv3x3_args(L, n, S, L.cout);
      ConvPlan fold{};                                   // (li == 1: the plan of the launch that carries the image layer)
      if (m.hook_split) {
        LRP_TRY(split_copy(S, (size_t)n * L.act_elems() / 8, st));
        ca.in = bufXs.as<float>(); ca.out_plain = 1;
      }
      ca.wpk = m.hook_split ? L.w_bwd_full_s.as<float>() : walk != 0 ? L.w_bwd_full.as<float>() : m.f16 ? L.w_bwd_h.as<float>()
               : m.split ? L.w_bwd_s.as<float>() : L.w_bwd.as<float>();
      ca.wpk_frag = m.f16 ? L.w_bwd_frag_h.as<float>() : (m.split && walk == 0) ? L.w_bwd_frag.as<float>() : nullptr;
      if (m.f16) {                                        // S_li (level li) -> S_{li-1} (level li - 1); the image layer ends the chain
        hipLaunchKernelGGL(tok_scale_kernel, dim3((n + 255) / 256), dim3(256), 0, st, lev_max(li), lev_exp(li),
                           L.wbs.as<float>(), tok_fac.as<float>(), li > 0 ? lev_exp(li - 1) : (int*)nullptr,
                           n, li == 0 ? 1 : 0);
        LRP_HIP_CHECK(hipGetLastError());
        ca.tok_fac = tok_fac.as<float>();
        if (li > 0) ca.tok_max_out = lev_max(li - 1);
      }
      ca.row2img = row2img_dev; ca.order = L.order.get(); ca.row2img_host = r2i_host;
      ca.gate_binary = walk != 0; ca.relu_out = walk == 3 || walk == 4;
      int epi;
      if (li == 0) {
        epi = image_layer_args(ca, n, Snext, R_img_dev, img_mode, 0.f, 0.f);
      } else {
        const ConvLayer& P = layers[li - 1];
        ca.N = L.cin; ca.aux = P.G.as<float>(); ca.out = Snext;
        epi = P.pool_after ? EPI_MUL_UP2 : EPI_MUL;
        if (walk == 4) {                                   // Deconvnet: the pool's routing, or nothing, in place of the ReLU gate
          if (P.pool_after) {
            LRP_TRY(position_gate(li - 1, st));
            ca.aux = P.Dg.as<float>();
          } else {
            ca.gate_none = 1;
          }
        }
        // the image layer rides on this launch's epilogue?
        if (li == 1 && m.fold_on && (fold = walk_plan(m, 1, pairs_in)).ok) {
          ca.img_w = P.w_bwd_s.as<float>(); ca.img_part = Snext; ca.out = nullptr;
        }
        if (pairs_in) {                                   // (ca.in = S stays a valid pointer; it is not read)
          ca.up2_src = S; ca.up2_pairs = 1; ca.up2_gpos = L.Gpos.as<unsigned char>();
          pairs_in = false;
        }
        if (writes_pairs(m, li)) {                         // THIS launch writes S_c for layer li - 1 (N = P.cin, at 2x this resolution)
          epi = EPI_MUL; ca.aux = P.Gc.as<float>();
          pairs_in = true;
        }
      }
      // PREC_F16X2: two MFMAs per product (the weights as ONE fp16, 11 bits) below the top block where a sum has at
      // least 576 products (64 channels), three (fp16 pairs on both sides) in the layers after the last pool.  [MI355X, bench configuration, relative L1 vs the float64 graph:
      // all layers three-term 2.8e-6 | two-term up to block4 3.1e-6 | two-term in block5 as well 9.7e-5 — the
      // relevance entering the top block is so concentrated that a sum has one or two dominant products and the
      // weight rounding, the same for every token, no longer averages out; profiles/r02_f16_terms_sweep.txt]
      // Encoder::two_term is that rule; lrp_set_fast_layers replaces it by a per-model mask, LRP_F16_T2MASK (experiments)
      // overrides both.
      const int terms = m.f16 && two_term(li) ? 5 : 7;
      if (epi == EPI_MUL_UP2) LRP_TRY(full_gate(li - 1, st));
      LRP_TRY(timed_conv(epi, ca, st, m.run_prec, layer_flop(n, li), terms));
      if (ca.img_part) return fold_image_sum(n, fold, ca.img_part, row2img_dev, R_img_dev, st);
      std::swap(S, Snext);
    }
    return image_stencil_tail(n, S, row2img_dev, R_img_dev, img_mode, 0.f, 0.f, st);   // (S now holds T)
  }
};

}  // namespace lrp

#include "encoder_weights.h"
#include "encoder_forward.h"
#include "encoder_rules.h"
#include "encoder_deeplift.h"
#include "encoder_trace.h"
#include "encoder_pattern.h"
