// encoder.h — host-side orchestration of the CNN half:
//   encode():  one forward per IMAGE, caching the relevance gates G_l and Z_top
//   explain(): one reverse walk per TOKEN (batched over all tokens of the call)
//   explain_deeplift(): the DeepLIFT walk against one reference image (lrp_set_deeplift_reference; deeplift_kernels.h)
//   explain_traced(): the LRP walk with the relevance at every layer's input kept and reduced (lrp_set_layer_trace; trace_kernels.h)
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
  // rule table (Encoder::set_table): the activator gate of a rule whose denominator is not the forward's Z+, the forward matrix of
  // that denominator (fp32, split8) and the layer's backward matrix over its one or two chains (cnn_kernels.h
  // pack_conv_rule_dev_kernel / pack_image_layer_rule_dev_kernel); for alpha-beta with beta > 0 the inhibitor gate
  // G- = a / safe(Z_inh) next to G (same mask) and the forward matrix w- of its denominator conv (fp32, split8).  Allocated by
  // the first table that needs them.
  DevBuf Gt, w_fwd_t, w_fwd_ts, w_bwd_t, w_bwd_t_s;
  DevBuf Gn, w_fwd_n, w_fwd_ns;
  bool t_packed = false;
  // DeepLIFT (Encoder::set_deeplift_reference): the reference's input and activation of this layer — ONE image's worth,
  // from the reference's own forward — and per image the gate D = M ? safe(Y - Yr) : 0 (deeplift_kernels.h dl_gate_kernel; every
  // layer, the top one included).  Allocated by the first reference that is set.
  DevBuf Xr, Yr, Dl;
  // PatternNet / PatternAttribution (Encoder::pattern_*): the fit's float64 sums [Sx | Sxy | cnt | Sy | P], the pattern
  // A (HWIO, as fitted or as set) and its packed copies for the walk's transposed conv — A and A * w in w_bwd_full's layout,
  // rebuilt by the next pattern walk after the pattern or the weights changed.  Allocated by the first pattern call that needs them.
  DevBuf pat_sums, pat, pat_bwd, pat_bwd_w;
  bool have_pat = false, pat_packed = false;
  size_t pat_sum_doubles() const { return (size_t)2 * 9 * cin * cout + 2 * (size_t)cout + 1; }
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
  // First layer whose ACTIVATION conv runs split-bf16 too.  A ~1e-5 relative error in a_l is harmless by itself, but
  // upstream of a 2x2 max-pool it flips the arg-max of near-tied windows (~1e-5 of them), and a flipped window moves
  // its whole relevance to a neighbour pixel: measured on VGG16, relative L1 of the heat-maps 5e-6 ... 3.6e-5 instead
  // of 5.6e-6.  Default: none (splitting only the layers behind the last pool is flip-free but makes the features the
  // decoder consumes 10x less exact, 7.4e-7 -> 7.8e-6, for 0.5 ms); lrp_set_precision(LRP_PREC_BF16X3_FAST): every layer
  // but the image layer (-5 ms, heat-map parity <= 4e-5): forward_fast.
  bool fwd_fast = false;
  // Activation chain and denominators in ONE pass on the fp16 MFMA: operands as fp16 pairs hi + lo (22 mantissa bits, x scaled by
  // a power of two per layer and image), product hi*hi' + hi*lo' + lo*hi' in three MFMAs with blocked fp32 accumulation,
  // weights (w | w+) stacked along N.
  // fp16-pair dual forward with interleaved weight rows: a_l and the gate G_l = a_l / safe(Z+_l) leave the conv's epilogue
  // together where no pool follows (conv_args.h ConvArgs::dual_il) — no Z+ tensor, no gate pass.  LRP_FWD_IL=0: stacked rows.
  static bool fwd_il() { return sw().fwd_il != 0; }
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

  // Fine-tune step: the weight gradient of layer l needs a_{l-1}; keep what the LRP caches drop.
  // Two users: the fine-tune step (for the life of the handle once lrp_train_begin ran) and a rule table (while it is set).
  // keep_acts = either; each asks and releases for itself, so neither can switch the other's activations off.
  // A DeepLIFT reference is a third user, while it is set and the handle is in LRP_PREC_FP32 (dl_active: its walk runs nowhere
  // else, and the other modes' forwards keep their fused forms); the layer trace (set_layer_trace) is a fourth, while it is on.
  // A pattern fit (pattern_fit_begin .. pattern_fit_end) is a fifth.  encode() decides keep_acts from the five.
  bool keep_acts = false, keep_for_train = false, keep_for_rule = false, keep_for_trace = false, keep_for_pattern = false;
  int alloc_keep_acts(int64_t* total) {
    for (size_t li = 0; li + 1 < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      if (!L.pool_after && !L.Akeep.p) LRP_TRY(L.Akeep.alloc((size_t)max_images * L.act_elems() * sizeof(float), total));   // (kept across a rule round trip)
    }
    return LRP_OK;
  }
  int enable_keep_acts(int64_t* total, bool for_rule = false) {
    LRP_TRY(alloc_keep_acts(total));
    (for_rule ? keep_for_rule : keep_for_train) = true;
    keep_acts = true;
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

  // ---- every operand copy is built ON THE DEVICE from the HWIO array in HBM: lrp_set_weight (the caller's host array is
  // copied there first), lrp_set_weight_dev (the multi-GPU start-up path: the bundle arrives over RCCL/xGMI and never
  // visits the host) and the fine-tune step (weights change every iteration).  "<name>_W" is split by sign (RR:256-260).
  DevBuf pack_tmp;                                     // scratch of the device packers (largest forward matrix)
  DevBuf f16_slots;                                    // ACT_MAX_SLOTS maxima while a weight matrix' fp16 copy is made
  int make_f16_operand(const float* src, size_t n_floats, int rows, int K, DevBuf& dst, DevBuf& wsc, int64_t* total, hipStream_t st) {
    return lrp::make_f16_operand(f16_slots, src, n_floats, rows, K, dst, wsc, total, st);      // f16_operand.h
  }
  int alloc_conv_operands(int li, int64_t* total, hipStream_t st) {
    ConvLayer& L = layers[li];
    auto mk = [&](DevBuf& d, size_t floats) -> int {
      if (d.p && d.bytes == floats * sizeof(float)) return LRP_OK;
      LRP_TRY(d.alloc(floats * sizeof(float), total));
      LRP_HIP_CHECK(hipMemsetAsync(d.p, 0, d.bytes, st));          // padding rows / columns stay zero
      return LRP_OK;
    };
    if (li == 0) {
      const size_t nb = (size_t)conv_npad(IMG_T_COLS) * conv_cinp(L.cout);
      LRP_TRY(mk(L.w_fwd, (size_t)conv_npad(2 * L.cout) * 64));
      if (image_layer_interleaved(L)) {
        LRP_TRY(mk(L.w_fwd_il, (size_t)conv_npad(2 * L.cout) * 64));
        LRP_TRY(mk(L.w_fwd_h, (size_t)conv_npad(2 * L.cout) * 64));
      } else {
        L.w_fwd_il.release();
      }
      LRP_TRY(mk(L.w_bwd, nb)); LRP_TRY(mk(L.w_bwd_s, nb)); LRP_TRY(mk(L.w_bwd_full, nb)); LRP_TRY(mk(L.w_bwd_h, nb));
      return LRP_OK;
    }
    const size_t Kf = (size_t)9 * conv_cinp(L.cin), Kb = (size_t)9 * conv_cinp(L.cout);
    const size_t nf = (size_t)conv_npad(L.cout) * Kf, nb = (size_t)conv_npad(L.cin) * Kb;
    LRP_TRY(mk(L.w_fwd, (size_t)conv_npad(2 * L.cout) * Kf)); LRP_TRY(mk(L.w_fwd_h, (size_t)conv_npad(2 * L.cout) * Kf));
    if (dual_interleaved(L)) LRP_TRY(mk(L.w_fwd_il, (size_t)conv_npad(2 * L.cout) * Kf));
    else L.w_fwd_il.release();
    LRP_TRY(mk(L.w_fwd_a, nf)); LRP_TRY(mk(L.w_fwd_zs, nf)); LRP_TRY(mk(L.w_fwd_as, nf));
    LRP_TRY(mk(L.w_bwd, nb)); LRP_TRY(mk(L.w_bwd_s, nb)); LRP_TRY(mk(L.w_bwd_full, nb)); LRP_TRY(mk(L.w_bwd_full_s, nb));
    LRP_TRY(mk(L.w_bwd_h, nb));
    if (L.sparse_ok() && L.idxp.p) LRP_TRY(mk(L.w_sp, conv_sparse_weight_floats(L.cin, L.cout)));
    // fragment-major copies, as large as the matrices they copy (VGG16's w_fwd_frag: 118 MB per handle), for every layer whose
    // launch can take a weights-in-registers form at some token / image count (conv_plan.h conv_frag_forms)
    if (conv_frag_forms(EPI_MUL, PREC_BF16X3, 7, L.cin, L.cout, 9)) LRP_TRY(mk(L.w_bwd_frag, nb));
    else L.w_bwd_frag.release();
    if (conv_frag_forms(EPI_MUL, PREC_F16X2, 7, L.cin, L.cout, 9)) LRP_TRY(mk(L.w_bwd_frag_h, nb));
    if (dual_interleaved(L) && conv_frag_forms(EPI_FWD_DUAL, PREC_F16X2, 7, 2 * L.cout, L.cin, 9)) LRP_TRY(mk(L.w_fwd_frag, (size_t)conv_npad(2 * L.cout) * Kf));
    else L.w_fwd_frag.release();
    if (pack_tmp.bytes < nf * sizeof(float)) LRP_TRY(pack_tmp.alloc(nf * sizeof(float), total));
    return LRP_OK;
  }
  // every operand copy of layer li from w_dev (HWIO, device); the buffers exist (alloc_conv_operands)
  int repack_conv_weight_from_device(int li, const float* w_dev, float* tmp, hipStream_t st) {
    ConvLayer& L = layers[li];
    if (li == 0) {
      const int Npb = conv_npad(IMG_T_COLS), Kb = conv_cinp(L.cout);
      hipLaunchKernelGGL(pack_image_layer_dev_kernel, dim3((27 * L.cout + 255) / 256), dim3(256), 0, st, w_dev, L.w_fwd.as<float>(),
                         L.w_bwd.as<float>(), L.w_bwd_full.as<float>(), L.cout, Kb);
      const size_t nb = (size_t)Npb * Kb;
      if (L.w_fwd_il.p) {
        hipLaunchKernelGGL(dual_interleave_rows_kernel, dim3(stream_grid((size_t)2 * L.cout * 64)), dim3(256), 0, st, L.w_fwd.as<float>(),
                           L.w_fwd_il.as<float>(), L.cout, 64);
        LRP_TRY(make_f16_operand(L.w_fwd_il.as<float>(), (size_t)conv_npad(2 * L.cout) * 64, 0, 0, L.w_fwd_h, L.wds, nullptr, st));
      }
      hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(nb / 8)), dim3(256), 0, st, L.w_bwd.as<float>(), L.w_bwd_s.as<float>(), nb / 8);
      LRP_TRY(make_f16_operand(L.w_bwd.as<float>(), nb, 0, 0, L.w_bwd_h, L.wbs, nullptr, st));
      LRP_HIP_CHECK(hipGetLastError());
      return LRP_OK;
    }
    const int CPi = conv_cinp(L.cin), CPo = conv_cinp(L.cout);
    const int Np2 = conv_npad(2 * L.cout), Npa = conv_npad(L.cout), Npb = conv_npad(L.cin);
    auto pack = [&](float* dst, int bwd, int rows, int dual, int pos) {
      const size_t tot = (size_t)rows * 9 * (bwd ? CPo : CPi);
      hipLaunchKernelGGL(pack_conv_dev_kernel, dim3(stream_grid(tot)), dim3(256), 0, st, w_dev, dst, bwd, L.cin, L.cout,
                         bwd ? CPo : CPi, rows, dual, pos);
    };
    auto split = [&](const float* src, float* dst, size_t n) {
      hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(n / 8)), dim3(256), 0, st, src, dst, n / 8);
    };
    const size_t nf = (size_t)Npa * 9 * CPi, nb = (size_t)Npb * 9 * CPo;
    pack(L.w_fwd.as<float>(), 0, Np2, 1, 0);
    if (L.w_fwd_il.p) pack(L.w_fwd_il.as<float>(), 0, Np2, 2, 0);
    LRP_TRY(make_f16_operand(L.w_fwd_il.p ? L.w_fwd_il.as<float>() : L.w_fwd.as<float>(), (size_t)Np2 * 9 * CPi, 0, 0, L.w_fwd_h,
                             L.wds, nullptr, st));
    if (L.w_fwd_frag.p)
      hipLaunchKernelGGL(pack_frag_dev_kernel, dim3(stream_grid((size_t)CPi / 32 * 9 * 8 * Np2)), dim3(256), 0, st, L.w_fwd_h.as<float>(),
                         L.w_fwd_frag.as<float>(), CPi, Np2);
    pack(L.w_fwd_a.as<float>(), 0, Npa, 0, 0);
    pack(tmp, 0, Npa, 0, 1);
    split(tmp, L.w_fwd_zs.as<float>(), nf);
    split(L.w_fwd_a.as<float>(), L.w_fwd_as.as<float>(), nf);
    pack(L.w_bwd.as<float>(), 1, Npb, 0, 1);
    split(L.w_bwd.as<float>(), L.w_bwd_s.as<float>(), nb);
    if (L.w_sp.p) LRP_HIP_CHECK(conv_sparse_pack(L.w_bwd.as<float>(), L.w_sp.as<float>(), L.cin, L.cout, st));
    if (L.w_bwd_frag.p)
      hipLaunchKernelGGL(pack_frag_dev_kernel, dim3(stream_grid((size_t)CPo / 32 * 9 * 8 * Npb)), dim3(256), 0, st, L.w_bwd_s.as<float>(),
                         L.w_bwd_frag.as<float>(), CPo, Npb);
    LRP_TRY(make_f16_operand(L.w_bwd.as<float>(), nb, Npb, 9 * CPo, L.w_bwd_h, L.wbs, nullptr, st));
    if (L.w_bwd_frag_h.p)
      hipLaunchKernelGGL(pack_frag_dev_kernel, dim3(stream_grid((size_t)CPo / 32 * 9 * 512)), dim3(256), 0, st, L.w_bwd_h.as<float>(),
                         L.w_bwd_frag_h.as<float>(), CPo, 64);
    pack(L.w_bwd_full.as<float>(), 1, Npb, 0, 0);
    split(L.w_bwd_full.as<float>(), L.w_bwd_full_s.as<float>(), nb);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }
  // fine-tune step: layer li (weights and bias) from the trainer's master buffer
  int repack_conv_from_device(int li, const float* w_dev, const float* b_dev, float* tmp, hipStream_t st) {
    ConvLayer& L = layers[li];
    if (!L.have_w || !L.have_b) return fail(LRP_ERR_STATE, "layer %d has no operand copies to rebuild", li);
    LRP_TRY(repack_conv_weight_from_device(li, w_dev, tmp, st));
    L.t_packed = false;
    L.pat_packed = false;
    if (table_on()) LRP_TRY(pack_table_layer(li, w_dev, st));
    L.norm_dirty = true;
    dl_ref_stale = true;
    LRP_HIP_CHECK(hipMemcpyAsync(L.bias.p, b_dev, (size_t)L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    L.raw_w_dev.release(); L.raw_b_dev.release();   // stale from here on (the trainer's master buffer is the truth)
    return LRP_OK;
  }
  // lrp_set_weight / lrp_set_weight_dev: "<name>_W" / "<name>_b" from host or device memory (`kind`) — one copy into
  // HBM, then the device packers; nothing here waits for the stream
  int set_conv_weight_dev(int li, const float* w, hipMemcpyKind kind, int64_t* total, hipStream_t st) {
    ConvLayer& L = layers[li];
    const size_t nW = (size_t)9 * L.cin * L.cout;
    if (gates_pending) {                               // the side stream may still read the operand copies we replace
      LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_gates, 0));
      gates_pending = false;
    }
    dl_ref_stale = true;                               // the reference's activations belong to the old weights
    if (!L.raw_w_dev.p) LRP_TRY(L.raw_w_dev.alloc(nW * sizeof(float), total));
    LRP_HIP_CHECK(hipMemcpyAsync(L.raw_w_dev.p, w, nW * sizeof(float), kind, st));
    LRP_TRY(alloc_conv_operands(li, total, st));
    LRP_TRY(repack_conv_weight_from_device(li, L.raw_w_dev.as<float>(), pack_tmp.as<float>(), st));
    L.have_w = true;
    L.norm_dirty = true;
    L.t_packed = false;                                // (repacked by the next encode under a rule table)
    L.pat_packed = false;                              // (A * w belongs to the old weights: repacked by the next pattern walk)
    encoded = 0;                                       // caches belong to the old weights
    return LRP_OK;
  }
  int set_conv_bias_dev(int li, const float* b, hipMemcpyKind kind, int64_t* total, hipStream_t st) {
    ConvLayer& L = layers[li];
    if (!L.raw_b_dev.p) LRP_TRY(L.raw_b_dev.alloc((size_t)L.cout * sizeof(float), total));
    if (!L.bias.p) LRP_TRY(L.bias.alloc((size_t)L.cout * sizeof(float), total));
    LRP_HIP_CHECK(hipMemcpyAsync(L.raw_b_dev.p, b, (size_t)L.cout * sizeof(float), kind, st));
    LRP_HIP_CHECK(hipMemcpyAsync(L.bias.p, L.raw_b_dev.p, (size_t)L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    L.have_b = true;
    L.norm_dirty = true;
    dl_ref_stale = true;
    encoded = 0;
    return LRP_OK;
  }

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
    keep_acts = keep_for_train || keep_for_rule || dl_active() || keep_for_trace || keep_for_pattern;
    if (dl_active() && dl_ref_stale) LRP_TRY(dl_reference_pass(st));
    ++encode_epoch;
    for (ConvLayer& L : layers) L.gfull_epoch = encode_epoch;     // (every path writes the full-resolution gates, except the fused pool: after_pool_gate)
    const size_t img_elems = (size_t)img_h * img_w * 3;
    if (gates_pending) {                               // the previous encode's side work still owns G / bufZ / bufXs
      LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_gates, 0));
      gates_pending = false;
    }
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
  static ConvArgs fwd_conv_args(const ConvLayer& L, int B, const float* in) {
    ConvArgs ca = conv3x3_args(L, B, in, L.cin);
    ca.bias = L.bias.as<float>();
    return ca;
  }
  // the image layer as a GEMM over its im2col matrix a1 (one row per pixel, 64 columns: 27 x+ | 27 x- | padding)
  int im2col_gemm_args(int B, hipStream_t st, ConvArgs& ca) {
    const ConvLayer& L = layers[0];
    const size_t total = (size_t)B * img_h * img_w * 8;
    hipLaunchKernelGGL(im2col_image_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       images.as<float>(), a1.as<float>(), B, img_h, img_w);
    LRP_HIP_CHECK(hipGetLastError());
    ca = ConvArgs{};
    ca.in = a1.as<float>(); ca.NB = B * L.H * L.W; ca.H = 1; ca.W = 1; ca.Cin = 64; ca.CinP = 64; ca.taps = 1;
    ca.bias = L.bias.as<float>();
    return LRP_OK;
  }
  // G_l = a_l / safe(Z+_l); may run in place (G == a)
  int gate_pass(ConvLayer& L, int B, const float* a, const float* z, hipStream_t st) {
    const size_t n = (size_t)B * L.act_elems();
    hipLaunchKernelGGL(gate_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(a),
                       reinterpret_cast<const f32x4*>(z), L.G.as<f32x4>(), n / 4);
    return launched();
  }
  // a_l where the gate pass of a layer finds it when the conv parked it in the gate's own storage
  const float* parked_act(const ConvLayer& L) const { return keep_acts ? L.Akeep.as<float>() : L.G.as<float>(); }
  // arg-max gate of a pooled layer at full resolution; pooled != nullptr: pool(a_l) as well
  int pool_gate_pass(ConvLayer& L, int B, const float* a, const float* z, float* pooled, hipStream_t st) {
    const size_t n = (size_t)B * L.act_elems();
    hipLaunchKernelGGL(pool_gate_kernel, dim3(stream_grid(n / 16)), dim3(256), 0, st, a, z, pooled, L.G.as<float>(), B, L.H, L.W, L.cout);
    return launched();
  }
  int maxpool_pass(ConvLayer& L, int B, const float* a, hipStream_t st) {
    const size_t n = (size_t)B * L.act_elems();
    hipLaunchKernelGGL(maxpool2_kernel, dim3(stream_grid(n / 16)), dim3(256), 0, st, a, L.P.as<float>(), B, L.H, L.W, L.cout);
    return launched();
  }
  int split_copy(const float* src, size_t n8, hipStream_t st) {      // split8 (bf16 hi | lo) copy of a conv input into bufXs
    hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(n8)), dim3(256), 0, st, src, bufXs.as<float>(), n8);
    return launched();
  }
  // where a layer's activation conv of the overlapped forwards writes a_l: the features, where the fine-tune step looks for
  // it, or parked in the storage of its future gate
  float* act_out(ConvLayer& L, bool top) { return top ? feat.as<float>() : (keep_acts && !L.pool_after) ? L.Akeep.as<float>() : L.G.as<float>(); }

  // One layer of the exact forward, and the image layer of every forward that does not emit: dual fp32 GEMM (a_l | Z+_l), gate
  // or pool-gate pass, x / a ping-pong.  On return x holds the next conv's input.
  int dual_fp32_layer(size_t li, int B, hipStream_t st, float*& x, float*& a, float* z) {
    ConvLayer& L = layers[li];
    const bool top = li + 1 == layers.size();
    ConvArgs ca;
    if (li == 0) LRP_TRY(im2col_gemm_args(B, st, ca));
    else ca = fwd_conv_args(L, B, x);
    ca.wpk = L.w_fwd.as<float>(); ca.N = 2 * L.cout; ca.split = L.cout;
    ca.out = top ? feat.as<float>() : a; ca.out2 = top ? ztop.as<float>() : z;
    if (dl_capture && li > 0)                            // the reference's forward: its input of this layer ...
      LRP_HIP_CHECK(hipMemcpyAsync(L.Xr.p, x, (size_t)L.H * L.W * L.cin * sizeof(float), hipMemcpyDeviceToDevice, st));
    LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, ca, st));
    if (dl_capture)                                      // ... and its activation, in front of the pool
      LRP_HIP_CHECK(hipMemcpyAsync(L.Yr.p, top ? feat.p : (void*)a, L.act_elems() * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (top) return LRP_OK;
    if (L.pool_after) {
      LRP_TRY(pool_gate_pass(L, B, a, z, x, st));      // x now holds pool(a): input of the next conv
    } else {
      LRP_TRY(gate_pass(L, B, a, z, st));
      std::swap(x, a);                                 // next input = a_l
    }
    if (keep_acts) {
      // these layers run through the ping-pong buffers: park the next conv's input where layer_input() looks for it
      const size_t bytes = (size_t)B * L.act_elems() * sizeof(float) / (L.pool_after ? 4 : 1);
      LRP_HIP_CHECK(hipMemcpyAsync(L.pool_after ? L.P.p : L.Akeep.p, x, bytes, hipMemcpyDeviceToDevice, st));
    }
    return LRP_OK;
  }

  // LRP_PREC_FP32, a width % 8 != 0 or a one-layer net (fwd_mode.h): everything on the caller's stream, exact fp32
  int forward_exact(int B, hipStream_t st) {
    float *x = bufX.as<float>(), *a = bufA.as<float>();
    for (size_t li = 0; li < layers.size(); ++li) LRP_TRY(dual_fp32_layer(li, B, st, x, a, bufZ.as<float>()));
    return LRP_OK;
  }

  // LRP_PREC_BF16X3_FAST: the caller's stream runs the activation chain a_1..a_top alone, split-bf16 behind the image layer (its
  // error passes through few further layers); the denominators and the gates follow on the side stream.
  int forward_fast(int B, hipStream_t st) {
    std::vector<const float*> xin(layers.size() + 1, nullptr);   // input of every conv
    float *x = bufX.as<float>(), *a = bufA.as<float>();
    LRP_TRY(dual_fp32_layer(0, B, st, x, a, bufZ.as<float>()));
    xin[1] = x;
    for (size_t li = 1; li < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      const bool top = li + 1 == layers.size();
      LRP_TRY(split_copy(xin[li], (size_t)B * L.H * L.W * L.cin / 8, st));
      ConvArgs ca = fwd_conv_args(L, B, bufXs.as<float>());
      ca.wpk = L.w_fwd_as.as<float>(); ca.N = L.cout; ca.out = act_out(L, top);
      LRP_HIP_CHECK(conv_launch(EPI_BIAS_RELU, ca, st, PREC_BF16X3));
      if (top) break;
      if (L.pool_after) LRP_TRY(maxpool_pass(L, B, ca.out, st));
      xin[li + 1] = L.pool_after ? L.P.as<float>() : ca.out;
    }
    // side stream, top layer first: layer l's input x_l = a_{l-1} lives in the gate storage of layer l-1, which
    // is turned into G_{l-1} only after layer l is done with it
    LRP_HIP_CHECK(hipEventRecord(ev_fwd, st));
    LRP_HIP_CHECK(hipStreamWaitEvent(side, ev_fwd, 0));
    for (size_t li = layers.size() - 1; li >= 1; --li) {
      ConvLayer& L = layers[li];
      const bool top = li + 1 == layers.size();
      LRP_TRY(split_copy(xin[li], (size_t)B * L.H * L.W * L.cin / 8, side));
      ConvArgs cz = fwd_conv_args(L, B, bufXs.as<float>());
      cz.wpk = L.w_fwd_zs.as<float>(); cz.N = L.cout; cz.out = top ? ztop.as<float>() : bufZ.as<float>();
      if (!top && !L.pool_after) {
        // no pool behind this layer: G_l = a_l / safe(Z+_l) in the conv's epilogue, Z+_l never written
        cz.gate_src = parked_act(L); cz.out = L.G.as<float>();
      }
      LRP_HIP_CHECK(conv_launch(EPI_BIAS, cz, side, PREC_BF16X3));
      if (!top && L.pool_after) LRP_TRY(pool_gate_pass(L, B, L.G.as<float>(), bufZ.as<float>(), nullptr, side));
    }
    LRP_HIP_CHECK(hipEventRecord(ev_gates, side));
    gates_pending = true;
    return LRP_OK;
  }

  // ---- fp16-pair dual forward (the default) ----
  // Scale records of layer / level `lev`: ACT_MAX_SLOTS maxima of its output, 2^-k of its input, 2^k of the pairs it emits.
  // `per` of each per layer: one for the whole batch, or — emitting — one per image, so that an image's result does not depend
  // on the rest of its batch.
  struct ScaleRecs {
    unsigned* max; float *unscale, *oscale; size_t per;
    unsigned* slots_of(size_t lev) const { return max + lev * per * ACT_MAX_SLOTS; }
    float* unscale_of(size_t li) const { return unscale + li * per; }
    float* oscale_of(size_t li) const { return oscale + li * per; }
  };
  ScaleRecs scale_recs(size_t per) const { return {act_max.as<unsigned>(), act_unscale.as<float>(), out_scale.as<float>(), per}; }
  // the dual conv a_l | Z+_l of layer li >= 1 over the pairs in `pin`; a_l goes to act_out, Z+_l to ztop / bufZ
  ConvArgs dual_pairs_args(size_t li, int B, const float* pin, const ScaleRecs& r, bool per_img) {
    ConvLayer& L = layers[li];
    const bool top = li + 1 == layers.size();
    ConvArgs cd = fwd_conv_args(L, B, pin);
    cd.wpk = L.w_fwd_h.as<float>(); cd.N = 2 * L.cout; cd.split = L.cout;
    cd.out = act_out(L, top); cd.out2 = top ? ztop.as<float>() : bufZ.as<float>();
    cd.in_unscale = r.unscale_of(li);
    cd.act_max_out = r.slots_of(li);
    cd.scale_per_img = per_img ? 1 : 0; cd.img_rows = L.H * L.W; cd.n_imgs = B;
    cd.dual_il = L.w_fwd_il.p ? 1 : 0;
    cd.wpk_frag = cd.dual_il ? L.w_fwd_frag.as<float>() : nullptr;
    return cd;
  }
  // no pool behind an interleaved layer: a_l and G_l leave the epilogue together — a_l into the ping-pong buffer its consumer
  // does not read from (or where the fine-tune step looks for it), the gate straight into its cache
  void fuse_gate(ConvLayer& L, ConvArgs& cd, const float* x_in) {
    if (!keep_acts) cd.out = x_in == bufA.as<float>() ? bufX.as<float>() : bufA.as<float>();
    cd.out2 = L.G.as<float>(); cd.dual_gate = 1;
  }
  // The denominators Z+_l of the layers whose reverse launch is two-term (explain(): up to the last pool, >= 576
  // products) are computed two-term as well — with the SAME rounded weights hi(w+) the walk multiplies with.
  // [MI355X: parity at the bench configuration 5.5e-6 -> 4.4e-6, 6 seeds median 4.2e-6 -> 3.3e-6: gate and
  // transposed conv now belong to one (slightly perturbed) network and the rounding largely cancels in R / Z+;
  // two-term Z+ in EVERY layer: 1.0e-4, the top block again.]
  int fwd_terms(size_t li, const ConvArgs& cd) const { return cd.dual_il && walk_f16 && two_term((int)li) ? 23 : 7; }
  // behind the pool gate of layer li, fused into the conv or a pass of its own: what this encode left for the walks
  int after_pool_gate(size_t li, int B, hipStream_t st, bool full_written) {
    ConvLayer& L = layers[li];
    if (L.Gc.p) L.gc_epoch = encode_epoch;
    if (!full_written) L.gfull_epoch = -1;             // G itself was not written: expanded on demand (full_gate)
    if (L.idxp.p && L.w_sp.p && sw().sparse_pool) {    // the sparse consumer's index words, once per image
      LRP_HIP_CHECK(conv_sparse_index(L.Gpos.as<unsigned char>(), L.idxp.as<unsigned>(), B, L.H / 2, L.W / 2, L.cout, st));
      L.idx_epoch = encode_epoch;
    }
    return LRP_OK;
  }

  // LRP_FWD_EMIT=0, or a layer without interleaved rows: one scale per batch; absmax (first conv), split, and — where the rows
  // are stacked — gate passes between the convs
  int forward_pairs_split(int B, hipStream_t st) {
    const ScaleRecs r = scale_recs(1);
    float* pin = bufXs.as<float>();
    float *x = bufX.as<float>(), *a = bufA.as<float>();
    LRP_TRY(dual_fp32_layer(0, B, st, x, a, bufZ.as<float>()));
    const float* x_in = x;                             // fp32 input of the conv about to run
    int gate_due = -1;                                 // layer whose gate waits for the next layer's split (it reads a_l)
    for (size_t li = 1; li < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      const bool top = li + 1 == layers.size();
      const size_t n8 = (size_t)B * L.H * L.W * L.cin / 8;
      if (li == 1)
        hipLaunchKernelGGL(absmax_slots_kernel, dim3(stream_grid(n8 * 2)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(x_in),
                           n8 * 2, r.slots_of(0));
      hipLaunchKernelGGL(split_h_scaled_kernel, dim3(stream_grid(n8)), dim3(256), 0, st, x_in, pin, n8, r.slots_of(li - 1),
                         r.unscale_of(li), L.wds.as<float>());
      LRP_HIP_CHECK(hipGetLastError());
      if (gate_due >= 0) {                             // a_{l-1} has been read: it may become G_{l-1} now
        LRP_TRY(gate_pass(layers[gate_due], B, parked_act(layers[gate_due]), bufZ.as<float>(), st));
        gate_due = -1;
      }
      ConvArgs cd = dual_pairs_args(li, B, pin, r, false);
      const bool fused_gate = cd.dual_il && !top && !L.pool_after;
      if (fused_gate) fuse_gate(L, cd, x_in);
      LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, cd, st, PREC_F16X2, fwd_terms(li, cd)));
      if (top) break;
      x_in = cd.out;
      if (L.pool_after) {
        LRP_TRY(maxpool_pass(L, B, cd.out, st));
        LRP_TRY(pool_gate_pass(L, B, L.G.as<float>(), bufZ.as<float>(), nullptr, st));
        x_in = L.P.as<float>();
      } else if (!fused_gate) {
        gate_due = (int)li;
      }
    }
    return LRP_OK;
  }

  // The default: the producer hands its consumer the fp16 pairs directly — the conv's epilogue where no pool follows, the fused
  // pool (or the pool pass) where one does; their scale comes from a bound that is known before the conv runs (fwd_scale_kernel:
  // the input's measured maximum times the layer's norm), the consumer's unscale with it.  No absmax, split or gate pass.
  int forward_pairs_emit(int B, hipStream_t st) {
    const ScaleRecs r = scale_recs((size_t)max_images);
    for (ConvLayer& L : layers) {
      if (!L.norm_dirty) continue;
      LRP_HIP_CHECK(hipMemsetAsync(L.fnorm.p, 0, 2 * sizeof(float), st));
      // (image layer: the a rows of its 64-wide im2col matrix hold w twice, against x+ and x-: the row sum is 2x the bound)
      const bool img = &L == &layers[0];
      hipLaunchKernelGGL(conv_norm_kernel, dim3(L.cout + 1), dim3(256), 0, st, img ? L.w_fwd.as<float>() : L.w_fwd_a.as<float>(), L.cout,
                         img ? 64 : 9 * conv_cinp(L.cin), L.bias.as<float>(), L.cout, L.fnorm.as<float>());
      LRP_HIP_CHECK(hipGetLastError());
      L.norm_dirty = false;
    }
    float *pin = bufXs.as<float>(), *pout = bufXl.as<float>();   // pin: the operand of the conv about to run
    LRP_TRY(image_layer_emit(B, st, r, pin));
    const float* x_in = keep_acts ? layers[0].Akeep.as<float>() : nullptr;   // where a_{l-1} went as fp32 (not read here)
    for (size_t li = 1; li < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      const bool top = li + 1 == layers.size();
      ConvArgs cd = dual_pairs_args(li, B, pin, r, true);
      if (!top) {
        hipLaunchKernelGGL(fwd_scale_kernel, dim3(B), dim3(64), 0, st, r.slots_of(li - 1), L.fnorm.as<float>(), layers[li + 1].wds.as<float>(),
                           r.oscale_of(li), r.unscale_of(li + 1));
        LRP_HIP_CHECK(hipGetLastError());
      }
      bool pool_fused = false;
      if (!top && !L.pool_after) {
        fuse_gate(L, cd, x_in);
        cd.pairs_out = pout; cd.pairs_scale = r.oscale_of(li); cd.skip_out = keep_acts ? 0 : 1;
      }
      const int fterms = fwd_terms(li, cd);
      if (!top && L.pool_after) {
        // max-pool, arg-max gate (compact form) and the pooled pairs in THIS conv's epilogue — a_l and Z+_l at full resolution
        // are neither written nor read back — where the launch takes the form that can (conv_plan)
        ConvAsk ask = conv_ask(EPI_FWD_DUAL, PREC_F16X2, fterms, false, cd);
        ask.pool_gc = true;
        pool_fused = !keep_acts && L.Gc.p && L.Gpos.p && conv_plan(ask).ok;
        if (pool_fused) {
          cd.pool_gc = L.Gc.as<float>(); cd.pool_pos = L.Gpos.as<unsigned char>(); cd.pairs_out = pout; cd.pairs_scale = r.oscale_of(li);
          cd.out = nullptr; cd.out2 = nullptr;
        }
      }
      LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, cd, st, PREC_F16X2, fterms));
      if (top) break;
      std::swap(pin, pout);
      x_in = L.pool_after ? L.P.as<float>() : cd.out;
      if (!L.pool_after) continue;
      if (!pool_fused) {
        // LRP_POOL_FUSED=0, the fine-tune step, or a launch that cannot pool: pooled activations as pairs (and fp32 only where
        // the fine-tune step looks for them) and the arg-max gate in one pass behind the conv
        const size_t n = (size_t)B * L.act_elems();
        hipLaunchKernelGGL(pool_gate_split_kernel, dim3(stream_grid(n / 32)), dim3(256), 0, st, L.G.as<float>(), bufZ.as<float>(),
                           L.G.as<float>(), pin, keep_acts ? L.P.as<float>() : (float*)nullptr, r.oscale_of(li), B, L.H, L.W, L.cout,
                           L.Gc.as<float>(), L.Gpos.as<unsigned char>());
        LRP_HIP_CHECK(hipGetLastError());
      }
      LRP_TRY(after_pool_gate(li, B, st, !pool_fused));
    }
    return LRP_OK;
  }

  // Image layer of the emitting forward: the fp32 GEMM over the im2col matrix with interleaved (w | w+-) rows — its epilogue
  // writes the gate G_1, a_1 as the next conv's fp16 pairs (scale from the images' measured maximum) and raises max|a_1|:
  // no gate / absmax / split pass, a_1 itself only where the fine-tune step looks for it.
  // (It stays on the exact fp32 MFMA: as fp16 pairs it is 0.2-0.4 ms faster per encode and puts the features of
  //  ill-conditioned nets at 1.0e-5 instead of 6.3e-6 — first-layer errors are inherited by every later layer.)
  int image_layer_emit(int B, hipStream_t st, const ScaleRecs& r, float* pairs_out) {
    ConvLayer& L = layers[0];
    unsigned* img_slots = r.slots_of(layers.size());
    hipLaunchKernelGGL(absmax_img_slots_kernel, dim3(64, B), dim3(256), 0, st, images.as<f32x4>(), (size_t)img_h * img_w * 3 / 4, img_slots);
    hipLaunchKernelGGL(fwd_scale_kernel, dim3(B), dim3(64), 0, st, img_slots, L.fnorm.as<float>(), layers[1].wds.as<float>(), r.oscale_of(0),
                       r.unscale_of(1));
    ConvArgs c0;
    LRP_TRY(im2col_gemm_args(B, st, c0));
    c0.wpk = L.w_fwd_il.as<float>(); c0.N = 2 * L.cout; c0.split = L.cout;
    c0.in_unscale = r.unscale_of(0);
    c0.dual_il = 1; c0.dual_gate = 1;
    c0.out = keep_acts ? L.Akeep.as<float>() : nullptr; c0.skip_out = keep_acts ? 0 : 1;
    c0.out2 = L.G.as<float>();
    c0.pairs_out = pairs_out; c0.pairs_scale = r.oscale_of(0);
    c0.act_max_out = r.slots_of(0);
    c0.scale_per_img = 1; c0.img_rows = L.H * L.W; c0.n_imgs = B;
    LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, c0, st));
    return LRP_OK;
  }

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

  // ---- rule table (lrp_set_cnn_rule, lrp_set_cnn_rules): one rule per conv ----
  // Layer l reads k_l relevance chains S_l = R_l / den_l — two for alpha-beta with beta > 0, one otherwise — as one tensor against one
  // tap-flipped matrix ([alpha w+ ; -beta w-], w+ or w) and applies the k_{l-1} gates of layer l-1's rule in its epilogue.
  // Alpha-beta with beta > 0 (RR:274-322) is R_in = alpha act - beta inh with two denominators per layer, Z_act (the Z+ of
  // alpha1beta0) and Z_inh = conv(x+, w-) + b (behind a ReLU or a pool x- = 0: the second conv of each branch contributes its bias
  // only).  Its chains S+ = R / safe(Z_act), S- = R / safe(Z_inh) travel as one tensor [S+ | S-] and every launch is ONE GEMM over both:
  //   c = convT(S+, alpha w+) + convT(S-, -beta w-);  S+' = G+ c,  S-' = G- c        (conv_args.h ConvArgs::aux_b)
  // — the dense dual-gate launches conv_plan answers for ConvAsk::dual_mul; the image layer is the same tap-expanded
  // GEMM + stencil over K = [S+ | S-].  Between rules of different chain counts: "two chains in, one gate" (the ordinary MUL epilogue
  // over Cin = 2 Cout) and "one chain in, two gates" (the dual-gate epilogue over Cin = Cout).  The gates that are not the forward's
  // come from table_pass at encode.
  // Dense launches only: no compact pool interface, no folded image layer, no sparse or weights-in-registers forms.
  struct ConvRule {
    int kind = LRP_RULE_ALPHA_BETA, bias = 1;
    float alpha = 1.f, beta = 0.f, eps = 0.f, low = 0.f, high = 0.f;
    int chains() const { return kind == LRP_RULE_ALPHA_BETA && beta > 0.f ? 2 : 1; }
    bool own_gate() const { return kind != LRP_RULE_ALPHA_BETA || !bias; }       // activator gate not the forward's a / safe(Z+)
    bool fwd_a() const { return (kind == LRP_RULE_ALPHA_BETA && !bias) || kind == LRP_RULE_BOUNDED; }   // ... and its denominator a conv with w+ | w-
    bool input_only() const { return kind == LRP_RULE_FLAT || kind == LRP_RULE_WSQUARE || kind == LRP_RULE_BOUNDED; }
  };
  // The handle's rule.  Empty: the default alpha1beta0 walk with all its fast forms — nothing below is allocated, launched or read.
  // Anything else, the same (alpha, beta > 0, bias) record on every conv (the one-rule entry) included, is a table.
  std::vector<ConvRule> table;
  DevBuf zt_top, wsq_zc;                               // the top layer's activator denominator where it is not ztop; w-square's border classes
  DevBuf a1b;                                          // BoundedRule: im2col of the image layer over (x - low | x - high) — a1 stays the forward's (the fine-tune step reads it)
  DevBuf zntop, s0ab, s1ab;                            // two chains: Z_inh of the top layer; the two-chain ping-pong
  bool table_on() const { return !table.empty(); }
  bool table_has_eps() const {
    for (const ConvRule& r : table)
      if (r.kind == LRP_RULE_EPSILON) return true;
    return false;
  }
  // epsilon kinds are exact-fp32 only (their gate a / (a + eps) is a step in a for small eps: a ReLU decision the fp16-pair forward
  // takes differently moves the map by O(1)); fp16 pairs have no table walk at all
  bool table_runs() const { return !walk_f16 && (!table_has_eps() || prec == PREC_FP32); }
  bool rule_split() const {                              // the table's arithmetic follows the handle's mode (as walk_mode's split)
    if (prec != PREC_BF16X3) return false;
    for (const ConvLayer& L : layers)
      if (L.cout & 7) return false;
    return true;
  }
  bool table_split() const { return rule_split() && !table_has_eps(); }
  void clear_table() {
    if (!table_on()) return;
    table.clear();
    keep_for_rule = false;                               // (the buffers stay, idle; the fine-tune step's own request stands)
    keep_acts = keep_for_train || keep_for_trace;
    encoded = 0;                                         // the caches belong to the old rule
  }
  // does layer li of `rules` walk on the default walk's own backward matrix (w+ tap-flipped; the image layer: w+ ; w-)?
  static bool rule_on_default_matrix(const ConvRule& r) { return r.kind == LRP_RULE_ALPHA_BETA && r.bias && r.chains() == 1; }
  static int table_chains(const std::vector<ConvRule>& rules) {
    int k = 1;
    for (const ConvRule& r : rules) k = std::max(k, r.chains());
    return k;
  }
  // `rules` is validated (engine.hip) and not empty
  int set_table(const std::vector<ConvRule>& rules, int64_t* total) {
    // a buffer appears, or grows, with the first table that needs it at that size: everything is sized by THIS table's chain counts
    auto mk = [&](DevBuf& d, size_t floats) -> int {
      if (d.p && d.bytes >= floats * sizeof(float)) return LRP_OK;
      if (d.p && total) *total -= (int64_t)d.bytes;
      LRP_TRY(d.alloc(floats * sizeof(float), total));
      LRP_HIP_CHECK(hipMemset(d.p, 0, d.bytes));
      return LRP_OK;
    };
    const size_t B = (size_t)max_images, NT = (size_t)max_tokens, nl = layers.size();
    for (size_t i = 0; i < nl; ++i) {
      ConvLayer& L = layers[i];
      const ConvRule& r = rules[i];
      const bool top = i + 1 == nl;
      const int k = r.chains();
      if (!top && r.own_gate()) LRP_TRY(mk(L.Gt, B * L.act_elems()));
      if (!top && k == 2) LRP_TRY(mk(L.Gn, B * L.act_elems()));
      const size_t nf = i == 0 ? (size_t)conv_npad(L.cout) * 64 : (size_t)conv_npad(L.cout) * 9 * conv_cinp(L.cin);
      const size_t nb = i == 0 ? (size_t)conv_npad(IMG_T_COLS) * conv_cinp(k * L.cout) : (size_t)conv_npad(L.cin) * 9 * conv_cinp(k * L.cout);
      if (r.fwd_a()) { LRP_TRY(mk(L.w_fwd_t, nf)); if (i) LRP_TRY(mk(L.w_fwd_ts, nf)); }
      if (k == 2) { LRP_TRY(mk(L.w_fwd_n, nf)); if (i) LRP_TRY(mk(L.w_fwd_ns, nf)); }
      if (!rule_on_default_matrix(r)) { LRP_TRY(mk(L.w_bwd_t, nb)); LRP_TRY(mk(L.w_bwd_t_s, nb)); }
      L.t_packed = false;
    }
    if (rules.back().own_gate()) LRP_TRY(mk(zt_top, B * layers.back().act_elems()));
    if (rules.back().chains() == 2) LRP_TRY(mk(zntop, B * layers.back().act_elems()));
    if (rules[0].kind == LRP_RULE_WSQUARE) LRP_TRY(mk(wsq_zc, (size_t)16 * layers[0].cout));
    if (rules[0].kind == LRP_RULE_BOUNDED) LRP_TRY(mk(a1b, B * img_h * img_w * 64));
    if (table_chains(rules) == 2) {                      // (one chain everywhere: the default walk's ping-pong s0 / s1)
      const size_t tok = std::max(2 * max_act_elems(), (size_t)img_h * img_w * IMG_T_COLS);
      LRP_TRY(mk(s0ab, NT * tok)); LRP_TRY(mk(s1ab, NT * tok));
    }
    LRP_TRY(enable_keep_acts(total, true));
    table = rules;
    encoded = 0;
    return LRP_OK;
  }
  // the table's operand copies of layer li from w_dev (HWIO, device)
  int pack_table_layer(int li, const float* w_dev, hipStream_t st) {
    ConvLayer& L = layers[li];
    const ConvRule& r = table[li];
    const int k = r.chains();
    auto split = [&](const float* src, float* dst, size_t n) {
      hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(n / 8)), dim3(256), 0, st, src, dst, n / 8);
    };
    const bool fwd_a = r.fwd_a();
    const bool own_bwd = !rule_on_default_matrix(r);
    if (own_bwd) {                                       // the last table's layout may have been another: cleared in stream order
      LRP_HIP_CHECK(hipMemsetAsync(L.w_bwd_t.p, 0, L.w_bwd_t.bytes, st));
      LRP_HIP_CHECK(hipMemsetAsync(L.w_bwd_t_s.p, 0, L.w_bwd_t_s.bytes, st));
    }
    if (li == 0) {
      const int Kb = conv_cinp(k * L.cout);
      if (!own_bwd) { L.t_packed = true; return LRP_OK; }   // (alpha-beta (1, 0) with bias needs nothing of its own)
      hipLaunchKernelGGL(pack_image_layer_rule_dev_kernel, dim3((27 * L.cout + 255) / 256), dim3(256), 0, st, w_dev,
                         fwd_a ? L.w_fwd_t.as<float>() : (float*)nullptr, k == 2 ? L.w_fwd_n.as<float>() : (float*)nullptr, L.w_bwd_t.as<float>(),
                         L.cout, Kb, r.kind, k, r.alpha, r.beta);
      split(L.w_bwd_t.as<float>(), L.w_bwd_t_s.as<float>(), (size_t)conv_npad(IMG_T_COLS) * Kb);
      if (r.kind == LRP_RULE_WSQUARE)
        hipLaunchKernelGGL(wsquare_class_kernel, dim3((16 * L.cout + 255) / 256), dim3(256), 0, st, w_dev, wsq_zc.as<float>(), L.cout);
    } else {
      const int CPi = conv_cinp(L.cin), CPk = conv_cinp(k * L.cout);
      const size_t nf = (size_t)conv_npad(L.cout) * 9 * CPi, nb = (size_t)conv_npad(L.cin) * 9 * CPk;
      auto pack = [&](float* dst, int bwd, int chains, float p0, float q0, float p1, float q1) {
        const int rows = bwd ? L.cin : L.cout, CP = bwd ? CPk : CPi;
        hipLaunchKernelGGL(pack_conv_rule_dev_kernel, dim3(stream_grid((size_t)rows * 9 * CP)), dim3(256), 0, st, w_dev, dst, bwd, L.cin, L.cout, CP,
                           rows, chains, p0, q0, p1, q1);
      };
      if (fwd_a) { pack(L.w_fwd_t.as<float>(), 0, 1, 1.f, 0.f, 0.f, 0.f); split(L.w_fwd_t.as<float>(), L.w_fwd_ts.as<float>(), nf); }
      if (k == 2) { pack(L.w_fwd_n.as<float>(), 0, 1, 0.f, 1.f, 0.f, 0.f); split(L.w_fwd_n.as<float>(), L.w_fwd_ns.as<float>(), nf); }
      if (own_bwd) {
        if (r.kind == LRP_RULE_EPSILON) pack(L.w_bwd_t.as<float>(), 1, 1, 1.f, 1.f, 0.f, 0.f);
        else if (k == 2) pack(L.w_bwd_t.as<float>(), 1, 2, r.alpha, 0.f, 0.f, -r.beta);
        else pack(L.w_bwd_t.as<float>(), 1, 1, 1.f, 0.f, 0.f, 0.f);          // (alpha-beta (1, 0) without the bias: w+)
        split(L.w_bwd_t.as<float>(), L.w_bwd_t_s.as<float>(), nb);
      }
    }
    LRP_HIP_CHECK(hipGetLastError());
    L.t_packed = true;
    return LRP_OK;
  }
  const float* table_gate(int li) const { return table[li].own_gate() ? layers[li].Gt.as<float>() : layers[li].G.as<float>(); }
  // Behind the forward (keep_acts: every conv's input is still there): per layer the denominators its rule needs beyond the forward's
  // Z+ — over the kept layer inputs, exact fp32 or three-term split-bf16 like the Z+ convs of the mixed modes with the handle
  // (epsilon tables: fp32; the image layer's GEMM stays fp32 as in every forward) — and the gates from them.  A pooled layer's
  // gates take the arg-max mask from G+; the top layer has no gate, its denominators stay next to ztop.
  int table_pass(int B, hipStream_t st) {
    if (gates_pending) {
      LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_gates, 0));
      gates_pending = false;
    }
    const bool split = table_split();
    for (size_t li = 0; li < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      const ConvRule& r = table[li];
      if (!L.t_packed) {
        if (!L.raw_w_dev.p) return fail(LRP_ERR_STATE, "layer '%s': set its weights again after a change of the CNN rule", L.name.c_str());
        LRP_TRY(pack_table_layer((int)li, L.raw_w_dev.as<float>(), st));
      }
      const bool top = li + 1 == layers.size();
      if (!top && L.pool_after) LRP_TRY(full_gate((int)li, st));
      // the gate a_l / safe(Z) of a layer with no pool behind it leaves the denominator conv's epilogue (ConvArgs::gate_src): Z
      // never goes to memory.  rule_gate_kernel's zmode 0 gives the same numbers, up to the sign of a zero where a_l = 0 and Z < 0.
      const bool fuse = !top && !L.pool_after;
      // one denominator conv: matrix (fp32, split8 or nullptr), bias or none; Z, or with `gated` the fused gate, into `dst`
      auto den_conv = [&](const float* w32, const float* ws, bool bias, bool bounded, float* dst, bool gated) -> int {
        ConvArgs cz;
        int zprec = PREC_FP32;
        if (li == 0 && bounded) {                        // its own im2col matrix: a1 stays what the forward built
          const size_t tot = (size_t)B * img_h * img_w * 8;
          hipLaunchKernelGGL(im2col_image_bounded_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, images.as<float>(),
                             a1b.as<float>(), B, img_h, img_w, r.low, r.high);
          LRP_HIP_CHECK(hipGetLastError());
          cz = ConvArgs{};
          cz.in = a1b.as<float>(); cz.NB = B * L.H * L.W; cz.H = 1; cz.W = 1; cz.Cin = 64; cz.CinP = 64; cz.taps = 1;
          cz.wpk = w32;
        } else if (li == 0) {
          LRP_TRY(im2col_gemm_args(B, st, cz));
          cz.wpk = w32;
        } else {
          const float* x = layer_input((int)li);
          if (split && ws) {
            LRP_TRY(split_copy(x, (size_t)B * L.H * L.W * L.cin / 8, st));
            x = bufXs.as<float>();
            zprec = PREC_BF16X3;
          }
          cz = fwd_conv_args(L, B, x);
          cz.wpk = zprec == PREC_BF16X3 ? ws : w32;
        }
        if (!bias) cz.bias = nullptr;
        cz.N = L.cout;
        cz.out = dst;
        if (gated) cz.gate_src = L.Akeep.as<float>();
        LRP_HIP_CHECK(conv_launch(EPI_BIAS, cz, st, zprec));
        return LRP_OK;
      };
      // gate from (value, denominator): a_l where no pool follows, the pooled activation under G+'s mask otherwise
      auto gate = [&](const float* z, int zmode, float* out) -> int {
        const size_t n4 = (size_t)B * L.act_elems() / 4;
        hipLaunchKernelGGL(rule_gate_kernel, dim3(stream_grid(n4)), dim3(256), 0, st, L.pool_after ? (const float*)nullptr : L.Akeep.as<float>(),
                           L.pool_after ? L.G.as<float>() : (const float*)nullptr, L.pool_after ? L.P.as<float>() : (const float*)nullptr, z,
                           wsq_zc.as<float>(), out, B, L.H, L.W, L.cout, zmode, r.eps);
        LRP_HIP_CHECK(hipGetLastError());
        return LRP_OK;
      };
      float* zbuf = bufZ.as<float>();
      if (r.own_gate()) {                                // the activator chain
        float* zdst = top ? zt_top.as<float>() : zbuf;
        float* gdst = fuse ? L.Gt.as<float>() : zdst;    // (a v / safe(z) gate)
        switch (r.kind) {
          case LRP_RULE_ALPHA_BETA:                      // without the bias: conv(x+, w+) + conv(x-, w-)
            LRP_TRY(den_conv(L.w_fwd_t.as<float>(), L.w_fwd_ts.as<float>(), false, false, gdst, fuse));
            if (!top && !fuse) LRP_TRY(gate(zbuf, 0, L.Gt.as<float>()));
            break;
          case LRP_RULE_BOUNDED:
            LRP_TRY(den_conv(L.w_fwd_t.as<float>(), nullptr, false, true, gdst, fuse));
            if (!top && !fuse) LRP_TRY(gate(zbuf, 0, L.Gt.as<float>()));
            break;
          case LRP_RULE_EPSILON:
            // behind a ReLU relevance arrives only where a > 0, and there Z = a with the bias: no conv.  The top layer's relevance
            // is the caller's, and without the bias Z is another sum: one conv with the full w (the exact activation conv's matrix;
            // the image layer: the w rows of its dual matrix)
            if (top || !r.bias) {
              LRP_TRY(den_conv(li == 0 ? L.w_fwd.as<float>() : L.w_fwd_a.as<float>(), nullptr, r.bias != 0, false, zdst, false));
              if (top) {
                const size_t nz = (size_t)B * L.act_elems();
                hipLaunchKernelGGL(stab_eps_kernel, dim3(stream_grid(nz)), dim3(256), 0, st, zdst, nz, r.eps);
                LRP_HIP_CHECK(hipGetLastError());
              } else {
                LRP_TRY(gate(zbuf, 1, L.Gt.as<float>()));
              }
            } else {
              LRP_TRY(gate(nullptr, 2, L.Gt.as<float>()));
            }
            break;
          case LRP_RULE_FLAT: LRP_TRY(gate(nullptr, 3, L.Gt.as<float>())); break;
          case LRP_RULE_WSQUARE: LRP_TRY(gate(nullptr, 4, L.Gt.as<float>())); break;
        }
      }
      if (r.chains() == 2) {                             // the inhibitor chain: conv(x+, w-) + conv(x-, w+), with the bias or without
        LRP_TRY(den_conv(L.w_fwd_n.as<float>(), L.w_fwd_ns.as<float>(), r.bias != 0, false,
                         top ? zntop.as<float>() : fuse ? L.Gn.as<float>() : zbuf, fuse));
        if (!top && L.pool_after) {
          const size_t n4 = (size_t)B * L.act_elems() / 4;
          hipLaunchKernelGGL(pool_gate_inh_kernel, dim3(stream_grid(n4)), dim3(256), 0, st, L.G.as<f32x4>(), L.P.as<float>(),
                             reinterpret_cast<const f32x4*>(zbuf), L.Gn.as<f32x4>(), B, L.H, L.W, L.cout);
          LRP_HIP_CHECK(hipGetLastError());
        }
      }
    }
    return LRP_OK;
  }
  // head of a rule's walk (KG:898-900 per chain): S_top = R / safe(den_top[img]) in the form the top layer's launch reads
  int rule_head(const ConvRule& r, bool split, int n, const int* row2img_dev, const float* R_feat_dev, float* S, hipStream_t st) {
    const ConvLayer& T = layers.back();
    const float* za = r.own_gate() ? zt_top.as<float>() : ztop.as<float>();
    const size_t pixels = (size_t)n * T.H * T.W, per = T.act_elems();
    if (r.chains() == 2) {
      const size_t items = pixels * (T.cout / (split ? 8 : 4));
      if (split)
        hipLaunchKernelGGL(chain_join_kernel<true>, dim3(stream_grid(items)), dim3(256), 0, st, R_feat_dev, R_feat_dev, za, zntop.as<float>(),
                           row2img_dev, S, pixels, T.H * T.W, T.cout);
      else
        hipLaunchKernelGGL(chain_join_kernel<false>, dim3(stream_grid(items)), dim3(256), 0, st, R_feat_dev, R_feat_dev, za, zntop.as<float>(),
                           row2img_dev, S, pixels, T.H * T.W, T.cout);
    } else if (split) {
      hipLaunchKernelGGL(top_divide_split_kernel, dim3(stream_grid((size_t)n * per / 8)), dim3(256), 0, st, R_feat_dev, za, row2img_dev, S, n, per / 8);
    } else {
      hipLaunchKernelGGL(top_divide_kernel, dim3(stream_grid((size_t)n * per / 4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(R_feat_dev),
                         reinterpret_cast<const f32x4*>(za), row2img_dev, reinterpret_cast<f32x4*>(S), n, per / 4);
    }
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }
  // the table's walk
  int explain_table(int n, const int* row2img_dev, const float* R_feat_dev, float* R_img_dev, hipStream_t st) {
    if (walk_f16) return fail(LRP_ERR_UNSUPPORTED, "LRP_PREC_F16X2 has no rule-table walk (its per-token scaling is per chain)");
    if (!table_runs()) return fail(LRP_ERR_UNSUPPORTED, "epsilon rules run in LRP_PREC_FP32 only");
    const bool split = table_split();
    const int rp = split ? PREC_BF16X3 : PREC_FP32;
    for (size_t li = 1; li < layers.size(); ++li) {      // every launch is one conv_plan answers: asked before the first one runs
      const ConvLayer& L = layers[li];
      ConvAsk q;
      q.epi = layers[li - 1].pool_after ? EPI_MUL_UP2 : EPI_MUL; q.prec = rp;
      q.NB = n; q.H = L.H; q.W = L.W; q.N = L.cin; q.Cin = table[li].chains() * L.cout; q.taps = 9;
      q.dual_mul = table[li - 1].chains() == 2;
      if (!conv_plan(q).ok)
        return fail(LRP_ERR_UNSUPPORTED, "conv %d: no launch reads %d chain(s) of %d channels into %d gate(s)", (int)li, table[li].chains(), L.cout,
                    table[li - 1].chains());
    }
    const bool two = table_chains(table) == 2;
    float *S = two ? s0ab.as<float>() : s0.as<float>(), *Snext = two ? s1ab.as<float>() : s1.as<float>();
    LRP_TRY(rule_head(table.back(), split, n, row2img_dev, R_feat_dev, S, st));
    const ConvRule& r0 = table[0];
    const int img_mode = r0.kind == LRP_RULE_ALPHA_BETA ? 0 : r0.kind == LRP_RULE_EPSILON ? 2 : r0.kind == LRP_RULE_BOUNDED ? 3 : 1;
    for (int li = (int)layers.size() - 1; li >= 0; --li) {
      const ConvLayer& L = layers[li];
      const int k = table[li].chains();
      ConvArgs ca = conv3x3_args(L, n, S, k * L.cout);
      if (rule_on_default_matrix(table[li])) ca.wpk = split ? L.w_bwd_s.as<float>() : L.w_bwd.as<float>();
      else ca.wpk = split ? L.w_bwd_t_s.as<float>() : L.w_bwd_t.as<float>();
      ca.row2img = row2img_dev;
      int epi;
      if (li == 0) {
        epi = image_layer_args(ca, n, Snext, R_img_dev, img_mode, r0.low, r0.high);
      } else {
        const ConvLayer& P = layers[li - 1];
        if (P.pool_after) LRP_TRY(full_gate(li - 1, st));
        ca.N = L.cin; ca.aux = table_gate(li - 1); ca.out = Snext;
        if (table[li - 1].chains() == 2) { ca.aux_b = P.Gn.as<float>(); ca.out_b = Snext + L.cin; ca.ostride = 2 * L.cin; }
        epi = P.pool_after ? EPI_MUL_UP2 : EPI_MUL;
      }
      prof.begin(st);
      LRP_HIP_CHECK(conv_launch(epi, ca, st, rp));
      prof.end(st, (double)k * layer_flop(n, li));
      std::swap(S, Snext);
    }
    return image_stencil_tail(n, S, row2img_dev, R_img_dev, img_mode, r0.low, r0.high, st);
  }

  // ---- DeepLIFT (lrp_set_deeplift_reference, LRP_WALK_DEEPLIFT; deeplift_kernels.h has the rule) ----
  // One reference image per handle.  At encode, in LRP_PREC_FP32: the reference goes through forward_exact as a batch of one (the
  // SAME path as the images: where image and reference agree on a receptive field Y and Yr are the same bits, which the dY == 0
  // branch of SafeDivide needs) whenever weights, precision or reference changed, keeping Xr_l / Yr_l; behind the images' own
  // forward dl_pass writes the gate D_l of every layer.  dX is not stored: the walk recomputes it from the kept layer inputs and
  // Xr_l (the same 4 bytes read per element and token as a stored dX, and no (images x activations) tensor per layer; Xr_l is one
  // image's worth and stays in L2).
  int dl_mode = 0;                                       // 0 off | 1 approximate_gradient=False (one chain) | 2 True (two chains + select)
  bool dl_ref_stale = true, dl_capture = false;
  long dl_epoch = -1;                                    // the encode whose gates D_l are current
  std::vector<float> dl_ref_host;                        // the reference as set, broadcast to (img_h, img_w, 3)
  DevBuf dl_s0, dl_s1, dl_r2i;                           // mode 2: the two chains' ping-pong (2 max_tokens rows) and row2img twice
  bool dl_active() const { return dl_mode != 0 && prec == PREC_FP32; }
  int set_deeplift_reference(const float* ref_host, float ref_scalar, int mode, int64_t* total) {
    if (mode == 0) {
      if (dl_mode != 0) { dl_mode = 0; encoded = 0; }    // (the buffers stay, idle)
      return LRP_OK;
    }
    const size_t img_elems = (size_t)img_h * img_w * 3;
    std::vector<float> ref(img_elems, ref_scalar);
    if (ref_host) ref.assign(ref_host, ref_host + img_elems);
    for (float v : ref)
      if (!(fabsf(v) < 3.0e38f)) return fail(LRP_ERR_INVALID, "the DeepLIFT reference must be finite");
    if (mode == dl_mode && ref == dl_ref_host) return LRP_OK;   // the same setting again changes nothing
    auto mk = [&](DevBuf& d, size_t bytes) -> int { return d.p && d.bytes >= bytes ? LRP_OK : d.alloc(bytes, total); };
    const size_t B = (size_t)max_images, NT = (size_t)max_tokens;
    for (ConvLayer& L : layers) {
      LRP_TRY(mk(L.Xr, (size_t)L.H * L.W * L.cin * sizeof(float)));
      LRP_TRY(mk(L.Yr, L.act_elems() * sizeof(float)));
      LRP_TRY(mk(L.Dl, B * L.act_elems() * sizeof(float)));
    }
    if (mode == 2) {                                     // (one chain: the default walk's ping-pong s0 / s1)
      const size_t tok = std::max(max_act_elems(), img_elems / 3 * IMG_T_COLS);
      LRP_TRY(mk(dl_s0, 2 * NT * tok * sizeof(float)));
      LRP_TRY(mk(dl_s1, 2 * NT * tok * sizeof(float)));
      LRP_TRY(mk(dl_r2i, 2 * NT * sizeof(int)));
    }
    LRP_TRY(alloc_keep_acts(total));
    LRP_HIP_CHECK(hipDeviceSynchronize());               // a walk in flight may still read the old reference
    LRP_HIP_CHECK(hipMemcpy(layers[0].Xr.p, ref.data(), img_elems * sizeof(float), hipMemcpyHostToDevice));
    dl_ref_host.swap(ref);
    dl_mode = mode;
    dl_ref_stale = true;
    encoded = 0;                                         // the caches belong to the old reference
    return LRP_OK;
  }
  // the reference's forward: image slot 0 and every cache it touches are overwritten by the encode that follows
  int dl_reference_pass(hipStream_t st) {
    if (gates_pending) {
      LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_gates, 0));
      gates_pending = false;
    }
    LRP_HIP_CHECK(hipMemcpyAsync(images.p, layers[0].Xr.p, (size_t)img_h * img_w * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    dl_capture = true;
    const int rc = forward_exact(1, st);
    dl_capture = false;
    LRP_TRY(rc);
    dl_ref_stale = false;
    return LRP_OK;
  }
  // behind the images' forward (keep_acts: every conv's input and activation is still there): the gates
  int dl_pass(int B, hipStream_t st) {
    for (size_t li = 0; li < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      const bool top = li + 1 == layers.size();
      const size_t n4 = (size_t)B * L.act_elems() / 4;
      if (L.pool_after) LRP_TRY(full_gate((int)li, st));
      const float* y = top ? feat.as<float>() : L.Akeep.as<float>();
      hipLaunchKernelGGL(dl_gate_kernel, dim3(stream_grid(n4)), dim3(256), 0, st, L.pool_after ? (const float*)nullptr : y,
                         L.pool_after ? L.G.as<float>() : (const float*)nullptr, L.pool_after ? L.P.as<float>() : (const float*)nullptr,
                         L.Yr.as<float>(), L.Dl.as<float>(), B, L.H, L.W, L.cout);
      LRP_HIP_CHECK(hipGetLastError());
    }
    dl_epoch = encode_epoch;
    return LRP_OK;
  }
  static int dl_combine(bool two, bool pool, const float* c, const float* x, const float* xr, const float* dn, const int* r2i, float* out, int n,
                        int H, int W, int C, hipStream_t st) {
    const dim3 grid(stream_grid((size_t)n * H * W * (C / 4)));
    if (two && pool) hipLaunchKernelGGL((dl_combine_kernel<true, true>), grid, dim3(256), 0, st, c, x, xr, dn, r2i, out, n, H, W, C);
    else if (two) hipLaunchKernelGGL((dl_combine_kernel<true, false>), grid, dim3(256), 0, st, c, x, xr, dn, r2i, out, n, H, W, C);
    else if (pool) hipLaunchKernelGGL((dl_combine_kernel<false, true>), grid, dim3(256), 0, st, c, x, xr, dn, r2i, out, n, H, W, C);
    else hipLaunchKernelGGL((dl_combine_kernel<false, false>), grid, dim3(256), 0, st, c, x, xr, dn, r2i, out, n, H, W, C);
    return launched();
  }
  static int dl_final(bool two, const float* c, const float* x, const float* xr, const int* r2i, float* out, int n, size_t per, hipStream_t st) {
    const bool v4 = !(per & 3);
    const dim3 grid(stream_grid((size_t)n * per / (v4 ? 4 : 1)));
    if (two && v4) hipLaunchKernelGGL((dl_final_kernel<true, 4>), grid, dim3(256), 0, st, c, x, xr, r2i, out, n, per);
    else if (two) hipLaunchKernelGGL((dl_final_kernel<true, 1>), grid, dim3(256), 0, st, c, x, xr, r2i, out, n, per);
    else if (v4) hipLaunchKernelGGL((dl_final_kernel<false, 4>), grid, dim3(256), 0, st, c, x, xr, r2i, out, n, per);
    else hipLaunchKernelGGL((dl_final_kernel<false, 1>), grid, dim3(256), 0, st, c, x, xr, r2i, out, n, per);
    return launched();
  }
  // The walk.  Per layer: the transposed conv with the full w (w_bwd_full, exact fp32, no gate in its epilogue) over the stacked
  // chains [t ; g] — 2n rows, n in mode 1 — then dl_combine_kernel: the select, the 2x routing through a pool and both gates of the
  // layer below.  The image layer is the stand-alone image launch over the same rows, then the select.
  int dl_check(int n) const {                            // mode before state: a refusal says what to change first
    if (n < 1 || n > max_tokens) return fail(LRP_ERR_INVALID, "n=%d outside [1,%d]", n, max_tokens);
    if (prec != PREC_FP32)
      return fail(LRP_ERR_UNSUPPORTED, "the DeepLIFT walk runs in LRP_PREC_FP32 only (dY of fp16-pair activations means nothing where it is small): "
                                       "set it with lrp_set_precision and call lrp_encode_images again");
    if (dl_mode == 0) return fail(LRP_ERR_STATE, "lrp_set_deeplift_reference must be called before the DeepLIFT walk");
    if (encoded < 1 || features_only || dl_epoch != encode_epoch)
      return fail(LRP_ERR_STATE, "lrp_encode_images must run (after lrp_set_deeplift_reference) before the DeepLIFT walk");
    return LRP_OK;
  }
  int explain_deeplift(int n, const int* row2img_dev, const float* head_dev, float* R_img_dev, hipStream_t st) {
    LRP_TRY(dl_check(n));
    const bool two = dl_mode == 2;
    const int rows = two ? 2 * n : n;
    float *S = two ? dl_s0.as<float>() : s0.as<float>(), *Snext = two ? dl_s1.as<float>() : s1.as<float>();
    const int* r2i_rows = row2img_dev;
    auto conv_args = [&](int li) {
      const ConvLayer& L = layers[li];
      ConvArgs ca = conv3x3_args(L, rows, S, L.cout);
      ca.wpk = L.w_bwd_full.as<float>();
      return ca;
    };
    // every launch is one conv_plan answers: asked before the first one runs
    for (int li = (int)layers.size() - 1; li >= 0; --li) {
      ConvArgs ca = conv_args(li);
      int epi = EPI_MUL;
      if (li == 0) epi = image_layer_args(ca, rows, Snext, Snext, 1, 0.f, 0.f);
      else ca.N = layers[li].cin;
      if (!conv_plan(conv_ask(epi, PREC_FP32, 7, false, ca)).ok)
        return fail(LRP_ERR_UNSUPPORTED, "conv %d: no exact-fp32 launch for %d rows of %d channels", li, rows, layers[li].cout);
    }
    if (two) {
      LRP_HIP_CHECK(hipMemcpyAsync(dl_r2i.p, row2img_dev, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
      LRP_HIP_CHECK(hipMemcpyAsync(dl_r2i.as<int>() + n, row2img_dev, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
      r2i_rows = dl_r2i.as<int>();
    }
    {
      const ConvLayer& T = layers.back();                // the head through the top layer's gates
      prof.begin(st);
      LRP_TRY(dl_combine(two, false, head_dev, nullptr, nullptr, T.Dl.as<float>(), row2img_dev, S, n, T.H, T.W, T.cout, st));
      prof.end(st, 0.0);
    }
    for (int li = (int)layers.size() - 1; li >= 1; --li) {
      const ConvLayer &L = layers[li], &P = layers[li - 1];
      ConvArgs ca = conv_args(li);
      ca.in = S; ca.N = L.cin; ca.out = Snext; ca.gate_none = 1;
      prof.begin(st);
      LRP_HIP_CHECK(conv_launch(EPI_MUL, ca, st, PREC_FP32));
      prof.end(st, (two ? 2.0 : 1.0) * layer_flop(n, li));
      prof.begin(st);
      LRP_TRY(dl_combine(two, P.pool_after, Snext, layer_input(li), L.Xr.as<float>(), P.Dl.as<float>(), row2img_dev, S, n, L.H, L.W, L.cin, st));
      prof.end(st, 0.0);
    }
    ConvArgs ca = conv_args(0);
    ca.in = S; ca.row2img = r2i_rows;
    const int epi = image_layer_args(ca, rows, Snext, Snext, 1, 0.f, 0.f);
    prof.begin(st);
    LRP_HIP_CHECK(conv_launch(epi, ca, st, PREC_FP32));
    prof.end(st, (two ? 2.0 : 1.0) * layer_flop(n, 0));
    const float* c = Snext;
    if (!img_fused()) {
      LRP_TRY(image_stencil_tail(rows, Snext, r2i_rows, S, 1, 0.f, 0.f, st));
      c = S;
    }
    prof.begin(st);
    LRP_TRY(dl_final(two, c, images.as<float>(), layers[0].Xr.as<float>(), row2img_dev, R_img_dev, n, (size_t)img_h * img_w * 3, st));
    prof.end(st, 0.0);
    return LRP_OK;
  }

  // ---- layer trace (lrp_set_layer_trace, lrp_cnn_explain_traced; trace_kernels.h has the arithmetic) ----
  // The reversed tensors of the reference's reverse analyzers: the head, and the relevance at the input of every node (conv or 2x2
  // pool, in execution order).  While the switch is on the handle is one more user of keep_acts; nothing else changes, and what the
  // traced walk needs beyond the rule's own buffers (the partials of its reductions) appears with the first traced call.
  struct TraceTensor {
    int nid, H, W, C;
    size_t elems() const { return (size_t)H * W * C; }
  };
  // in sorted-id order: (-1, 0) the head, (0, 0) the image, ...
  std::vector<TraceTensor> trace_tensors() const {
    std::vector<TraceTensor> v;
    v.push_back(TraceTensor{-1, top_h, top_w, top_c});
    int nid = 0;
    for (const ConvLayer& L : layers) {
      v.push_back(TraceTensor{nid++, L.H, L.W, L.cin});
      if (L.pool_after) v.push_back(TraceTensor{nid++, L.H, L.W, L.cout});
    }
    return v;
  }
  // index (in trace_tensors) of the input tensor of conv li; the pool behind conv li follows the conv's own
  int trace_index_of_conv(int li) const {
    int t = 1;
    for (int q = 0; q < li; ++q) t += layers[q].pool_after ? 2 : 1;
    return t;
  }
  // where the tensors `mask` selects lie in a keep buffer for n rows (floats; every tensor starts on a multiple of 4): -1 for the
  // others.  Returns the buffer's size.
  int64_t trace_keep_layout(int n, uint64_t mask, std::vector<int64_t>& off) const {
    const std::vector<TraceTensor> tt = trace_tensors();
    off.assign(tt.size(), -1);
    int64_t cur = 0;
    for (size_t t = 0; t < tt.size(); ++t) {
      if (!((mask >> t) & 1)) continue;
      off[t] = cur;
      cur += ((int64_t)n * (int64_t)tt[t].elems() + 3) / 4 * 4;
    }
    return cur;
  }
  int set_layer_trace(bool on, int64_t* total) {
    if (on == keep_for_trace) return LRP_OK;             // the same setting again changes nothing
    if (on) LRP_TRY(alloc_keep_acts(total));
    keep_for_trace = on;
    encoded = 0;                                         // the next encode keeps (or stops keeping) the layer inputs
    return LRP_OK;
  }
  static const ConvRule& default_rule() {
    static const ConvRule r;
    return r;
  }
  const ConvRule& rule_at(int li) const { return table_on() ? table[li] : default_rule(); }
  int trace_check(int n) const {                         // mode before state, as dl_check
    if (n < 1 || n > max_tokens) return fail(LRP_ERR_INVALID, "n=%d outside [1,%d]", n, max_tokens);
    if (walk_f16) return fail(LRP_ERR_UNSUPPORTED, "LRP_PREC_F16X2 has no traced walk (its chains travel under per-token scales)");
    if (table_on() && !table_runs()) return fail(LRP_ERR_UNSUPPORTED, "epsilon rules run in LRP_PREC_FP32 only");
    if (!keep_for_trace) return fail(LRP_ERR_STATE, "lrp_set_layer_trace(h, 1) must be called before lrp_cnn_explain_traced");
    if (encoded < 1 || features_only) return fail(LRP_ERR_STATE, "lrp_encode_images must run (after lrp_set_layer_trace) before lrp_cnn_explain_traced");
    return LRP_OK;
  }
  DevBuf tr_part;                                        // [2 tensors][max_tokens][chunks of the largest layer][TRACE_PART] doubles
  static int trace_chunks(const ConvLayer& L, bool split) {
    const size_t items = (size_t)L.H * L.W * (L.cin / (split ? 8 : 4));
    return (int)((items + TRACE_ITEMS_PER_BLOCK - 1) / TRACE_ITEMS_PER_BLOCK);
  }
  static int tensor_stats(const float* x, int rows, size_t per_row, double* stats, hipStream_t st) {
    hipLaunchKernelGGL(tensor_stats_kernel, dim3(rows), dim3(1024), 0, st, x, per_row, stats);
    return launched();
  }
  static int trace_layer(bool pool, bool split, int k, const TraceLayerArgs& t, int nblk, hipStream_t st) {
    const dim3 grid(nblk, t.n);
#define LRP_TRACE_CASE(P, S, K) \
  if (pool == P && split == S && k == K) hipLaunchKernelGGL((trace_layer_kernel<P, S, K>), grid, dim3(256), 0, st, t)
    LRP_TRACE_CASE(false, false, 1); LRP_TRACE_CASE(false, false, 2); LRP_TRACE_CASE(false, true, 1); LRP_TRACE_CASE(false, true, 2);
    LRP_TRACE_CASE(true, false, 1); LRP_TRACE_CASE(true, false, 2); LRP_TRACE_CASE(true, true, 1); LRP_TRACE_CASE(true, true, 2);
#undef LRP_TRACE_CASE
    return launched();
  }
  // stats_dev (n_tensors, n, 4) float64; keep_dev with `keep_off` from trace_keep_layout (nullptr: nothing is kept)
  int explain_traced(int n, const int* row2img_dev, const float* R_feat_dev, float* R_img_dev, double* stats_dev, float* keep_dev,
                     const std::vector<int64_t>& keep_off, hipStream_t st) {
    LRP_TRY(trace_check(n));
    if (gates_pending) LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_gates, 0));   // gates / Z_top come from the side stream
    const bool split = table_on() ? table_split() : rule_split();
    const int rp = split ? PREC_BF16X3 : PREC_FP32;
    const int nl = (int)layers.size();
    bool two = false;
    for (int li = 0; li < nl; ++li) two = two || rule_at(li).chains() == 2;
    float *S = two ? s0ab.as<float>() : s0.as<float>(), *Snext = two ? s1ab.as<float>() : s1.as<float>();
    const ConvRule& r0 = rule_at(0);
    const int img_mode = r0.kind == LRP_RULE_ALPHA_BETA ? 0 : r0.kind == LRP_RULE_EPSILON ? 2 : r0.kind == LRP_RULE_BOUNDED ? 3 : 1;
    auto conv_args = [&](int li) {
      const ConvLayer& L = layers[li];
      ConvArgs ca = conv3x3_args(L, n, S, rule_at(li).chains() * L.cout);
      if (rule_on_default_matrix(rule_at(li))) ca.wpk = split ? L.w_bwd_s.as<float>() : L.w_bwd.as<float>();
      else ca.wpk = split ? L.w_bwd_t_s.as<float>() : L.w_bwd_t.as<float>();
      ca.row2img = row2img_dev;
      if (li > 0) { ca.N = L.cin; ca.out = Snext; ca.gate_none = 1; ca.out_plain = 1; }
      return ca;
    };
    // every launch is one conv_plan answers: asked before the first one runs
    int max_chunks = 1;
    for (int li = nl - 1; li >= 0; --li) {
      ConvArgs ca = conv_args(li);
      int epi = EPI_MUL;
      if (li == 0) epi = image_layer_args(ca, n, Snext, R_img_dev, img_mode, r0.low, r0.high);
      else max_chunks = std::max(max_chunks, trace_chunks(layers[li], false));   // (sized for either arithmetic: it never grows)
      if (!conv_plan(conv_ask(epi, rp, 7, false, ca)).ok)
        return fail(LRP_ERR_UNSUPPORTED, "conv %d: no launch reads %d chain(s) of %d channels into a plain accumulator", li, rule_at(li).chains(),
                    layers[li].cout);
    }
    const size_t part_row = (size_t)max_chunks * TRACE_PART, part_tensor = (size_t)max_tokens * part_row;
    if (!tr_part.p) LRP_TRY(tr_part.alloc(2 * part_tensor * sizeof(double), ws_total));
    const std::vector<TraceTensor> tt = trace_tensors();
    auto keep_ptr = [&](int t) -> float* { return keep_dev && keep_off[(size_t)t] >= 0 ? keep_dev + keep_off[(size_t)t] : nullptr; };
    auto stats_of = [&](int t) { return stats_dev + (size_t)t * n * 4; };
    auto whole = [&](int t, const float* x) -> int {     // a tensor that exists as such: the head, the image
      LRP_TRY(tensor_stats(x, n, tt[(size_t)t].elems(), stats_of(t), st));
      if (float* k = keep_ptr(t)) LRP_HIP_CHECK(hipMemcpyAsync(k, x, (size_t)n * tt[(size_t)t].elems() * sizeof(float), hipMemcpyDeviceToDevice, st));
      return LRP_OK;
    };
    LRP_TRY(whole(0, R_feat_dev));
    LRP_TRY(rule_head(rule_at(nl - 1), split, n, row2img_dev, R_feat_dev, S, st));
    for (int li = nl - 1; li >= 1; --li) {
      const ConvLayer &L = layers[li], &P = layers[li - 1];
      const int k = rule_at(li - 1).chains();
      prof.begin(st);
      LRP_HIP_CHECK(conv_launch(EPI_MUL, conv_args(li), st, rp));
      prof.end(st, (double)rule_at(li).chains() * layer_flop(n, li));
      if (P.pool_after) LRP_TRY(full_gate(li - 1, st));
      const int tc = trace_index_of_conv(li), nblk = trace_chunks(L, split);
      TraceLayerArgs t{};
      t.acc = Snext; t.a = layer_input(li); t.gpos = P.pool_after ? P.G.as<float>() : nullptr;
      t.g0 = table_on() ? table_gate(li - 1) : P.G.as<float>(); t.g1 = k == 2 ? P.Gn.as<float>() : nullptr;
      t.row2img = row2img_dev; t.S = S;
      t.keep_conv = keep_ptr(tc); t.keep_pool = P.pool_after ? keep_ptr(tc - 1) : nullptr;
      t.part_conv = tr_part.as<double>(); t.part_pool = tr_part.as<double>() + part_tensor;
      t.n = n; t.H = L.H; t.W = L.W; t.C = L.cin;
      prof.begin(st);
      LRP_TRY(trace_layer(P.pool_after, split, k, t, nblk, st));
      prof.end(st, 0.0);
      hipLaunchKernelGGL(trace_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, t.part_conv, n, nblk, stats_of(tc));
      if (P.pool_after) hipLaunchKernelGGL(trace_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, t.part_pool, n, nblk, stats_of(tc - 1));
      LRP_HIP_CHECK(hipGetLastError());
    }
    ConvArgs ca = conv_args(0);
    const int epi = image_layer_args(ca, n, Snext, R_img_dev, img_mode, r0.low, r0.high);
    prof.begin(st);
    LRP_HIP_CHECK(conv_launch(epi, ca, st, rp));
    prof.end(st, (double)r0.chains() * layer_flop(n, 0));
    LRP_TRY(image_stencil_tail(n, Snext, row2img_dev, R_img_dev, img_mode, r0.low, r0.high, st));
    return whole(1, R_img_dev);
  }

  // ---- PatternNet / PatternAttribution (lrp_pattern_*, LRP_WALK_PATTERNNET / _PATTERN_ATTRIBUTION; pattern_kernels.h) ----
  // The fit and the walk are independent: the walk takes whatever patterns the layers hold, fitted here or set by the caller.
  // Everything below is allocated by the first pattern call that needs it; a handle that never makes one allocates nothing.
  int pat_type = -1;                                     // the running fit's mask (PAT_*), -1: no fit is open
  long pat_fit_epoch = -1, pat_batches = 0;              // the encode accumulated last; batches accumulated by this fit
  bool pat_project = true;                               // reverse_project_bottleneck_layers (pattern_based.py:175-183)
  DevBuf pat_prod, pat_ws, pat_part;                     // fit: the batch's two products (fp32), the K-split workspace, the mask pass' partials
  size_t pat_ws_floats = 0;
  DevBuf pat_div, pat_maxpart;                           // walk: a row's divisor, the partials of its maximum
  int pattern_mode_check() const {
    if (prec != PREC_FP32)
      return fail(LRP_ERR_UNSUPPORTED, "the pattern fit and walks run in LRP_PREC_FP32 only (a mask taken in another arithmetic is another mask): "
                                       "set it with lrp_set_precision and call lrp_encode_images again");
    return LRP_OK;
  }
  int pattern_fit_begin(int type, int64_t* total) {
    if (type < PAT_LINEAR || type > PAT_RELU_NEGATIVE) return fail(LRP_ERR_INVALID, "unknown pattern type %d", type);
    LRP_TRY(pattern_mode_check());
    size_t max_kc = 0, max_cout = 0;
    for (const ConvLayer& L : layers) {
      max_kc = std::max(max_kc, (size_t)9 * L.cin * L.cout);
      max_cout = std::max(max_cout, (size_t)L.cout);
    }
    if ((size_t)27 * layers[0].cout * sizeof(float) > 65536)
      return fail(LRP_ERR_UNSUPPORTED, "the image layer's fit holds 27 x cout weights in LDS: cout <= 592");
    auto mk = [&](DevBuf& d, size_t bytes) -> int { return d.p && d.bytes >= bytes ? LRP_OK : d.alloc(bytes, total); };
    for (ConvLayer& L : layers) LRP_TRY(mk(L.pat_sums, L.pat_sum_doubles() * sizeof(double)));
    LRP_TRY(mk(pat_prod, 2 * max_kc * sizeof(float)));
    pat_ws_floats = 8 * max_kc;
    LRP_TRY(mk(pat_ws, pat_ws_floats * sizeof(float)));
    LRP_TRY(mk(pat_part, (size_t)PAT_MAX_CHUNKS * 2 * max_cout * sizeof(double)));
    LRP_TRY(alloc_keep_acts(total));
    LRP_HIP_CHECK(hipDeviceSynchronize());               // (an earlier fit's launches may still add to the sums)
    for (ConvLayer& L : layers) LRP_HIP_CHECK(hipMemset(L.pat_sums.p, 0, L.pat_sum_doubles() * sizeof(double)));
    LRP_HIP_CHECK(hipDeviceSynchronize());
    pat_type = type; pat_fit_epoch = -1; pat_batches = 0;
    keep_for_pattern = true;
    encoded = 0;                                         // the next encode keeps the layer inputs
    return LRP_OK;
  }
  int pattern_fit_check() const {
    LRP_TRY(pattern_mode_check());
    if (pat_type < 0) return fail(LRP_ERR_STATE, "lrp_pattern_fit_begin must be called first");
    return LRP_OK;
  }
  // the images of the last encode: per conv c = conv(x) + b, the mask pass, the two products, the float64 sums
  int pattern_fit_batch(hipStream_t st) {
    LRP_TRY(pattern_fit_check());
    if (encoded < 1 || features_only || !keep_acts)
      return fail(LRP_ERR_STATE, "lrp_encode_images must run (after lrp_pattern_fit_begin) before lrp_pattern_fit_batch");
    if (pat_fit_epoch == encode_epoch) return fail(LRP_ERR_STATE, "this encode is already part of the fit: an encode is accumulated at most once");
    const int B = encoded;
    float *c = bufA.as<float>(), *m = bufZ.as<float>(), *ym = bufXs.as<float>();
    auto conv_args = [&](int li) {
      ConvArgs ca = fwd_conv_args(layers[li], B, layer_input(li));
      ca.wpk = layers[li].w_fwd_a.as<float>(); ca.N = layers[li].cout; ca.out = c;
      return ca;
    };
    // every launch is one conv_plan answers: asked before the first one runs
    for (int li = 1; li < (int)layers.size(); ++li)
      if (!conv_plan(conv_ask(EPI_BIAS, PREC_FP32, 7, false, conv_args(li))).ok)
        return fail(LRP_ERR_UNSUPPORTED, "conv %d: no exact-fp32 launch for its pre-activation", li);
    for (int li = 0; li < (int)layers.size(); ++li) {
      const ConvLayer& L = layers[li];
      const long P = (long)B * L.H * L.W;
      const size_t KC = (size_t)9 * L.cin * L.cout;
      prof.begin(st);
      if (li == 0) {
        hipLaunchKernelGGL(pattern_image_conv_kernel, dim3(stream_grid((size_t)P * (L.cout / 4))), dim3(256), (size_t)27 * L.cout * sizeof(float), st,
                           images.as<float>(), L.w_fwd.as<float>(), L.bias.as<float>(), c, B, L.H, L.W, L.cout);
        LRP_HIP_CHECK(hipGetLastError());
      } else {
        LRP_HIP_CHECK(conv_launch(EPI_BIAS, conv_args(li), st, PREC_FP32));
      }
      prof.end(st, 2.0 * (double)P * (double)KC);
      const long rows_per = std::max(256L, (P + PAT_MAX_CHUNKS - 1) / PAT_MAX_CHUNKS);
      const int chunks = (int)((P + rows_per - 1) / rows_per);
      prof.begin(st);
      hipLaunchKernelGGL(pattern_mask_kernel, dim3(chunks), dim3(256), 0, st, c, L.bias.as<float>(), m, ym, pat_part.as<double>(), P, L.cout,
                         rows_per, pat_type);
      LRP_HIP_CHECK(hipGetLastError());
      prof.end(st, 0.0);
      SgemmArgs a{};                                     // X^T . rhs, all nine taps in one launch (the weight gradient's product)
      a.A = layer_input(li); a.lda = L.cin; a.ldb = L.cout; a.ldc = L.cout;
      a.M = L.cin; a.N = L.cout; a.K = P; a.transA = 1; a.transB = 0;
      a.gather = 1; a.gH = L.H; a.gW = L.W; a.taps = 9; a.tapC = (long)L.cin * L.cout;
      prof.begin(st);
      a.B = m; a.C = pat_prod.as<float>();
      LRP_HIP_CHECK(sgemm(a, pat_ws.as<float>(), pat_ws_floats, st));
      a.B = ym; a.C = pat_prod.as<float>() + KC;
      LRP_HIP_CHECK(sgemm(a, pat_ws.as<float>(), pat_ws_floats, st));
      prof.end(st, 4.0 * (double)P * (double)KC);
      prof.begin(st);
      hipLaunchKernelGGL(pattern_accumulate_kernel, dim3(stream_grid(2 * KC)), dim3(256), 0, st, pat_prod.as<float>(), pat_part.as<double>(), chunks,
                         L.pat_sums.as<double>(), KC, L.cout, (double)P);
      LRP_HIP_CHECK(hipGetLastError());
      prof.end(st, 0.0);
    }
    pat_fit_epoch = encode_epoch;
    ++pat_batches;
    return LRP_OK;
  }
  int pattern_alloc(ConvLayer& L) {
    if (!L.pat.p) LRP_TRY(L.pat.alloc((size_t)9 * L.cin * L.cout * sizeof(float), ws_total));
    return LRP_OK;
  }
  // sums -> patterns, installed; the fit is closed (its sums stay readable until the next lrp_pattern_fit_begin)
  int pattern_fit_end(hipStream_t st) {
    LRP_TRY(pattern_fit_check());
    if (pat_batches < 1) return fail(LRP_ERR_STATE, "lrp_pattern_fit_batch must run at least once before lrp_pattern_fit_end");
    for (ConvLayer& L : layers) LRP_TRY(pattern_alloc(L));
    for (size_t li = 0; li < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      const int CP = li == 0 ? 0 : conv_cinp(L.cin);
      hipLaunchKernelGGL(pattern_compute_kernel, dim3(L.cout), dim3(256), 0, st, L.pat_sums.as<double>(),
                         li == 0 ? L.w_fwd.as<float>() : L.w_fwd_a.as<float>(), li == 0 ? 64 : 9 * CP, CP, L.cin, L.cout, L.pat.as<float>());
      LRP_HIP_CHECK(hipGetLastError());
      L.have_pat = true;
      L.pat_packed = false;
    }
    pat_type = -1;
    keep_for_pattern = false;                            // (the caches of the last encode stay valid: they hold more than is needed)
    return LRP_OK;
  }
  int pattern_set(int li, const float* A_dev, hipStream_t st) {
    ConvLayer& L = layers[li];
    LRP_TRY(pattern_alloc(L));
    LRP_HIP_CHECK(hipMemcpyAsync(L.pat.p, A_dev, (size_t)9 * L.cin * L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    L.have_pat = true;
    L.pat_packed = false;
    return LRP_OK;
  }
  // the walk's matrices of every layer whose pattern or weights changed: A and A * w as the gradient walk's w_bwd_full is packed
  int pattern_pack(hipStream_t st) {
    for (size_t li = 0; li < layers.size(); ++li) {
      ConvLayer& L = layers[li];
      if (L.pat_packed) continue;
      const size_t nb = li == 0 ? (size_t)conv_npad(IMG_T_COLS) * conv_cinp(L.cout) : (size_t)conv_npad(L.cin) * 9 * conv_cinp(L.cout);
      for (DevBuf* d : {&L.pat_bwd, &L.pat_bwd_w}) {
        if (d->p && d->bytes == nb * sizeof(float)) continue;
        LRP_TRY(d->alloc(nb * sizeof(float), ws_total));
        LRP_HIP_CHECK(hipMemsetAsync(d->p, 0, d->bytes, st));          // padding rows / columns stay zero
      }
      if (li == 0) {
        hipLaunchKernelGGL(pattern_pack_image_kernel, dim3((27 * L.cout + 255) / 256), dim3(256), 0, st, L.pat.as<float>(), L.pat_bwd.as<float>(),
                           L.cout, conv_cinp(L.cout));
      } else {
        const int CPo = conv_cinp(L.cout), Npb = conv_npad(L.cin);
        hipLaunchKernelGGL(pack_conv_dev_kernel, dim3(stream_grid(nb)), dim3(256), 0, st, L.pat.as<float>(), L.pat_bwd.as<float>(), 1, L.cin,
                           L.cout, CPo, Npb, 0, 0);
      }
      hipLaunchKernelGGL(pattern_mul_kernel, dim3(stream_grid(nb / 4)), dim3(256), 0, st, L.pat_bwd.as<f32x4>(), L.w_bwd_full.as<f32x4>(),
                         L.pat_bwd_w.as<f32x4>(), nb / 4);
      LRP_HIP_CHECK(hipGetLastError());
      L.pat_packed = true;
    }
    return LRP_OK;
  }
  int pattern_walk_check(int n) const {                  // mode before state, as dl_check
    if (n < 1 || n > max_tokens) return fail(LRP_ERR_INVALID, "n=%d outside [1,%d]", n, max_tokens);
    LRP_TRY(pattern_mode_check());
    for (const ConvLayer& L : layers)
      if (!L.have_pat) return fail(LRP_ERR_STATE, "conv '%s' has no pattern: fit them (lrp_pattern_fit_*) or set them (lrp_set_patterns)", L.name.c_str());
    if (encoded < 1 || features_only) return fail(LRP_ERR_STATE, "lrp_encode_images must run before the pattern walk");
    return LRP_OK;
  }
  // a row's divisor: max |x| of each of the n rows of x, 1 where that is 0
  int pattern_row_div(const float* x, int n, size_t per_row, hipStream_t st) {
    const int chunks = pattern_chunks(per_row);
    hipLaunchKernelGGL(pattern_absmax_part_kernel, dim3(chunks, n), dim3(256), 0, st, x, per_row, pat_maxpart.as<float>());
    hipLaunchKernelGGL(pattern_absmax_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, pat_maxpart.as<float>(), n, chunks, pat_div.as<float>());
    return launched();
  }
  // The walk (pattern_based.py:68-125): per conv + ReLU layer the ReLU's gradient, then the conv's gradient with the kernel replaced
  // by A (PatternNet) or A * w (PatternAttribution); every reversed tensor is divided by its row's absolute maximum first
  // (pat_project; the head, every conv's input, the result — behind a pool the routed tensor's maximum is already 1).
  int explain_pattern(int n, const int* row2img_dev, const float* head_dev, float* R_img_dev, bool attribution, hipStream_t st) {
    LRP_TRY(pattern_walk_check(n));
    if (gates_pending) LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_gates, 0));
    const int nl = (int)layers.size();
    float *S = s0.as<float>(), *Snext = s1.as<float>();
    auto matrix = [&](int li) { return attribution ? layers[li].pat_bwd_w.as<float>() : layers[li].pat_bwd.as<float>(); };
    auto conv_args = [&](int li) {
      const ConvLayer& L = layers[li];
      ConvArgs ca = conv3x3_args(L, n, S, L.cout);
      ca.wpk = matrix(li); ca.row2img = row2img_dev;
      if (li > 0) { ca.N = L.cin; ca.out = Snext; ca.gate_none = 1; ca.out_plain = 1; }
      return ca;
    };
    // every launch is one conv_plan answers: asked before the first one runs
    const size_t img_row = (size_t)img_h * img_w * 3;
    int max_chunks = std::max(pattern_chunks(layers.back().act_elems()), pattern_chunks(img_row));
    for (int li = nl - 1; li >= 0; --li) {
      ConvArgs ca = conv_args(li);
      int epi = EPI_MUL;
      if (li == 0) epi = image_layer_args(ca, n, Snext, R_img_dev, 1, 0.f, 0.f);
      else max_chunks = std::max(max_chunks, pattern_chunks((size_t)layers[li].H * layers[li].W * layers[li].cin));
      if (!conv_plan(conv_ask(epi, PREC_FP32, 7, false, ca)).ok)
        return fail(LRP_ERR_UNSUPPORTED, "conv %d: no exact-fp32 launch reads %d channels into a plain accumulator", li, layers[li].cout);
    }
    if (!pat_div.p) {
      LRP_TRY(pat_div.alloc((size_t)max_tokens * sizeof(float), ws_total));
      LRP_TRY(pat_maxpart.alloc((size_t)max_tokens * max_chunks * sizeof(float), ws_total));
    }
    LRP_TRY(pattern_pack(st));
    const float* div = pat_project ? pat_div.as<float>() : nullptr;
    {
      const ConvLayer& T = layers.back();                // the head, projected, through the top ReLU
      const size_t per4 = T.act_elems() / 4;
      prof.begin(st);
      if (pat_project) LRP_TRY(pattern_row_div(head_dev, n, T.act_elems(), st));
      hipLaunchKernelGGL(pattern_head_kernel, dim3(stream_grid((size_t)n * per4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(head_dev),
                         feat.as<f32x4>(), row2img_dev, div, reinterpret_cast<f32x4*>(S), n, per4);
      LRP_HIP_CHECK(hipGetLastError());
      prof.end(st, 0.0);
    }
    for (int li = nl - 1; li >= 1; --li) {
      const ConvLayer &L = layers[li], &P = layers[li - 1];
      prof.begin(st);
      LRP_HIP_CHECK(conv_launch(EPI_MUL, conv_args(li), st, PREC_FP32));
      prof.end(st, layer_flop(n, li));
      if (P.pool_after) LRP_TRY(full_gate(li - 1, st));
      PatternProjectArgs t{};
      t.acc = Snext; t.gate = P.G.as<float>(); t.row2img = row2img_dev; t.div = div; t.S = S;
      t.n = n; t.H = L.H; t.W = L.W; t.C = L.cin;
      prof.begin(st);
      if (pat_project) LRP_TRY(pattern_row_div(Snext, n, (size_t)L.H * L.W * L.cin, st));
      const dim3 grid(stream_grid((size_t)n * L.H * L.W * (L.cin / 4)));
      if (P.pool_after) hipLaunchKernelGGL((pattern_project_kernel<true>), grid, dim3(256), 0, st, t);
      else hipLaunchKernelGGL((pattern_project_kernel<false>), grid, dim3(256), 0, st, t);
      LRP_HIP_CHECK(hipGetLastError());
      prof.end(st, 0.0);
    }
    ConvArgs ca = conv_args(0);
    const int epi = image_layer_args(ca, n, Snext, R_img_dev, 1, 0.f, 0.f);
    prof.begin(st);
    LRP_HIP_CHECK(conv_launch(epi, ca, st, PREC_FP32));
    prof.end(st, layer_flop(n, 0));
    LRP_TRY(image_stencil_tail(n, Snext, row2img_dev, R_img_dev, 1, 0.f, 0.f, st));
    if (pat_project) {
      prof.begin(st);
      LRP_TRY(pattern_row_div(R_img_dev, n, img_row, st));
      hipLaunchKernelGGL(pattern_scale_kernel, dim3(stream_grid((size_t)n * img_row / 4)), dim3(256), 0, st, R_img_dev, img_row, pat_div.as<float>(), n);
      LRP_HIP_CHECK(hipGetLastError());
      prof.end(st, 0.0);
    }
    return LRP_OK;
  }

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
    if (n < 1 || n > max_tokens) return fail(LRP_ERR_INVALID, "n=%d outside [1,%d]", n, max_tokens);
    if (walk < 0 || walk > 4) return fail(LRP_ERR_INVALID, "unknown walk %d", walk);
    if (encoded < 1 || features_only) return fail(LRP_ERR_STATE, "lrp_encode_images must run before the CNN explain");
    if (gates_pending) LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_gates, 0));   // gates / Z_top come from the side stream
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
      prof.begin(st);
      LRP_HIP_CHECK(conv_launch(epi, ca, st, m.run_prec, terms));
      prof.end(st, layer_flop(n, li));
      if (ca.img_part) return fold_image_sum(n, fold, ca.img_part, row2img_dev, R_img_dev, st);
      std::swap(S, Snext);
    }
    return image_stencil_tail(n, S, row2img_dev, R_img_dev, img_mode, 0.f, 0.f, st);   // (S now holds T)
  }
};

}  // namespace lrp
