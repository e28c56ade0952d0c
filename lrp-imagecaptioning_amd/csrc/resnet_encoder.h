// resnet_encoder.h — host-side orchestration of the CNN half for the ResNet-101 encoder (BASELINE config 4:
// grid-TD decoder + ResNet-101 cut at conv5_block3_out, LRP-alpha1beta0).  Same contract as Encoder (encoder.h):
//   encode():  one forward per IMAGE, caching per conv unit the gate that combines the BatchNorm reverse rule
//              (RA:197-257) with the alpha1beta0 denominator (RR:274-322) and per block the Add-rule factors (RA:260-286)
//   explain(): one reverse walk per TOKEN: three (four) convs per bottleneck block on conv_igemm + streaming kernels
// The algorithm is oracle/resnet_lrp_ref.analyze_cached, which equals the literal iNNvestigate walk to 1e-10.
// This path runs in exact fp32 (PREC_FP32) throughout.
//   explain_ab(): the same walk under the alpha-beta rule with beta > 0 (set_rule): two relevance chains per tensor, the second
//              gate of every unit and block made at encode time behind the unchanged forward (oracle: tests/resnet_ab_ref.py).
//   set_rules(): the rule PAIR — one record for the stem conv, one for every conv above it (alpha-beta / epsilon with or without the
//              bias; flat, w-square, bounded at the stem).  rule_gates() writes the pair's gates behind the unchanged forward,
//              explain() / explain_ab() walk them by the unit record's chain count, stem_end() ends both by the stem record's
//              (oracle: tests/resnet_rule_ref.py).
//   explain_grad(): the gradient family, one walk driven by a GradMode.  Gradient / InputTimesGradient / GuidedBackprop in
//              LRP_PREC_FP32 mode: the same convT launches with BN-scaled full-sign weights (w_g, packed on the first such walk)
//              and the ReLU decisions the fp32 forward recorded as byte masks (RnUnit::mask, RnBlock::omask).  Deconvnet: the
//              guided walk without any mask (a clamp at every Activation, no ReLU decision read; the stem pool by pool_win),
//              every precision mode.
// What the paths share, each written once:
//   encode() = the common part + encode_emit() (fp16 pairs between the convs) or encode_fp32_acts() (fp32 activations between
//              them); both start with stem_forward() and build a unit's launch from fwd_args(), bn_epilogue() and
//              launch_inh_dual()
//   bwd_args(): the transposed conv through a unit over one or two chains (unit_backward, explain_ab, grad_backward)
//   stem_reverse(): the tap GEMM + stencil, or the fused kernel where it applies, behind all three walks
//   reserve() / split_copy(): the buffers and split8 copies of the packers (pack_unit_dev, set_rule, ensure_*_weights)
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "conv_launch.h"
#include "conv_plan.h"
#include "f16_operand.h"
#include "resnet_kernels.h"

namespace lrp {

constexpr float RN_BN_EPS = 1.001e-5f;

struct RnUnit {            // conv + BN
  std::string name;
  int k = 1, cin = 0, cout = 0, stride = 1;
  int Hin = 0, Win = 0, Hout = 0, Wout = 0;
  bool relu = false;
  bool have[6] = {false, false, false, false, false, false};   // W b gamma beta mean var
  DevBuf w_a, w_z, w_b, w_bs, bias, gamma, beta, mean, var;   // w_bs: w_b in split8 form (bf16x3 reverse walk)
  DevBuf w_dual;   // [w rows | w+ rows]: c and Z+ of the unit in one conv pass (EPI_FWD_DUAL without the relu)
  DevBuf w_dual_h, wds;    // w_dual as fp16 pairs scaled by a power of two + its scale record (f16_operand.h)
  bool dual_il = false;    // ... with its rows interleaved per 32 channels ([w | w+] side by side): BN + gate in the conv's epilogue
  DevBuf gate;             // [B][Hout][Wout][cout]: act*Q (relu units) or Q (pre-Add units)
  // gradient walks: [B][Hout][Wout][cout] bytes, y > 0 (relu units behind the stem; written by the LRP_PREC_FP32 forward), and the
  // backward matrix of conv + BN (w_b's layout, full sign, W * gamma / sqrt(var + eps)), packed on the first gradient walk after a
  // weight of the unit changed (grad_ok)
  DevBuf mask, w_g;
  bool grad_ok = false;
  // alpha-beta rule with beta > 0 (ResNetEncoder::set_rule; none of these exists before the first such rule): the inhibitor gate
  // (gate's form with Zi = conv(x, w-) + b), the forward matrix of Zi (w_n: w- in w_a's layout; the stem: the swapped-slot matrix;
  // w_dualn_h: interleaved [w | w-] fp16 pairs of a dual_il unit) and the backward matrix [alpha w+ ; -beta w-], plain and split8
  DevBuf gate_i, w_n, w_dualn_h, w_ab, w_abs;
  bool ab_packed = false;
  // rule pair (ResNetEncoder::set_rules): the one-chain backward matrix of a rule that does not walk on w_b — the full w of the
  // epsilon kinds; the stem: w, 1 or w^2 in the T+ rows, those two in split8 form as well.  Neither exists before the first such rule
  DevBuf w_r, w_rs;
  bool rule_packed = false;
  size_t out_elems() const { return (size_t)Hout * Wout * cout; }
  size_t in_elems() const { return (size_t)Hin * Win * cin; }
};

struct RnBlock {
  int u0 = -1, u1 = -1, u2 = -1, u3 = -1;     // unit indices (u0 = projection shortcut or -1)
  int stride = 1, cin = 0, f = 0, Hin = 0, Win = 0, H = 0, W = 0;
  DevBuf t_in;             // [B][Hin][Win][cin] block input (what relevance is multiplied with at the fork)
  DevBuf t_sub;            // [B][H][W][cin] stride-2 gather of t_in (first block of stacks 3..5)
  DevBuf GA, GS;           // [B][H][W][4f]: fA*Q3 and fS (identity) / fS*Q0 (projection)
  DevBuf omask;            // [B][H][W][4f] bytes: block output > 0 (LRP_PREC_FP32 forward; the gradient walks)
  DevBuf GA_i, GS_i;       // fA*Q3i and (projection blocks) fS*Q0i: the inhibitor chain's GA / GS (beta > 0)
};

struct ResNetEncoder {
  int img_h = 0, img_w = 0, max_images = 0, max_tokens = 0, stem_c = 0;
  int top_h = 0, top_w = 0, top_c = 0;
  std::vector<RnUnit> units;       // units[0] = stem
  std::vector<RnBlock> blocks;
  DevBuf images, stemA, a0;        // image copy, stem im2col, stem activation [B][H/2][W/2][stem]
  // the stem's routing needs Q alone: what arrives at a0 = relu(y) through the pool is already a relevance
  // (t * C1 of the first block), so multiplying by the relu-unit gate a0*Q would count a0 twice
  DevBuf q_stem;
  DevBuf pool_win;                 // winner of every 3x3/2 pool window (one byte)
  const void* stem_attr_set[8] = {};   // the rn_stem_reverse_kernel instantiations whose LDS attribute is set (stem_lds_attr)
  DevBuf fa, fb, fc, fz, fsc;      // forward scratch
  DevBuf fxs;                      // a unit's input as scaled fp16 pairs (fp16-pair forward)
  DevBuf f16_slots;                // scratch maxima of make_f16_operand
  DevBuf act_max, act_unscale;     // ACT_MAX_SLOTS maxima per unit output / block output; 2^-k per unit input
  // round-4 forward (encode_emit): per IMAGE max-slots of every unit / block output, the pair scale of every tensor that is
  // written as pairs, the unscale of every unit's input, and per unit the bound constants {A, B} (rn_unit_norm_kernel)
  DevBuf eslots, eoscale, eunscale, fnorm;
  bool norms_ready = false;
  DevBuf feat;                     // [B][top...]
  DevBuf r0, r1, r2, r3, r4, r5;   // reverse scratch (per token)
  int encoded = 0;
  bool features_only = false;
  int prec = PREC_BF16X3;  // arithmetic of the reverse walk's conv chains (lrp_set_precision); forward stays exact fp32
  bool masks_ok = false;   // the ReLU masks belong to the current encode (an LRP_PREC_FP32 forward)
  int64_t* ws_total = nullptr;   // the handle's workspace counter (lazy allocations of the gradient walks)
  Profiler prof;           // one record per unit_backward launch (common.h)

  int add_unit(const std::string& nm, int k, int cin, int cout, int stride, int Hin, int Win, bool relu) {
    RnUnit u;
    u.name = nm; u.k = k; u.cin = cin; u.cout = cout; u.stride = stride; u.Hin = Hin; u.Win = Win; u.relu = relu;
    u.Hout = (Hin + stride - 1) / stride; u.Wout = (Win + stride - 1) / stride;
    units.push_back(std::move(u));
    return (int)units.size() - 1;
  }

  int init(const lrp_config& c, int64_t* total) {
    img_h = c.img_h; img_w = c.img_w; max_images = c.max_images; max_tokens = c.max_tokens; stem_c = c.resnet_stem;
    ws_total = total;
    if (c.resnet_n_stacks < 1 || c.resnet_n_stacks > 8) return fail(LRP_ERR_INVALID, "resnet_n_stacks out of range");
    if ((img_h % 4) || (img_w % 4) || stem_c % 4) return fail(LRP_ERR_UNSUPPORTED, "image size and stem width must be multiples of 4");
    add_unit("conv1", 7, 3, stem_c, 2, img_h, img_w, true);
    int H = img_h / 4, W = img_w / 4, cin = stem_c;
    for (int s = 0; s < c.resnet_n_stacks; ++s) {
      const int f = c.resnet_filters[s], nb = c.resnet_blocks[s];
      if (f % 4 || nb < 1) return fail(LRP_ERR_INVALID, "bad resnet stack %d", s);
      for (int b = 1; b <= nb; ++b) {
        char nm[64];
        snprintf(nm, sizeof(nm), "conv%d_block%d", s + 2, b);
        const int stride = (b == 1 && s > 0) ? 2 : 1;
        if (stride == 2 && ((H & 1) || (W & 1))) return fail(LRP_ERR_UNSUPPORTED, "odd resolution before a stride-2 block");
        RnBlock B;
        B.stride = stride; B.cin = cin; B.f = f; B.Hin = H; B.Win = W; B.H = H / stride; B.W = W / stride;
        if (b == 1) B.u0 = add_unit(std::string(nm) + "_0", 1, cin, 4 * f, stride, H, W, false);
        B.u1 = add_unit(std::string(nm) + "_1", 1, cin, f, stride, H, W, true);
        B.u2 = add_unit(std::string(nm) + "_2", 3, f, f, 1, B.H, B.W, true);
        B.u3 = add_unit(std::string(nm) + "_3", 1, f, 4 * f, 1, B.H, B.W, false);
        blocks.push_back(std::move(B));
        H /= stride; W /= stride; cin = 4 * f;
      }
    }
    top_h = H; top_w = W; top_c = cin;
    if (top_h * top_w != c.L || top_c != c.D)
      return fail(LRP_ERR_INVALID, "ResNet output (%d x %d x %d) does not match L=%d, D=%d", top_h, top_w, top_c, c.L, c.D);
    const size_t B = max_images, NT = max_tokens;
    size_t max_act = (size_t)(img_h / 2) * (img_w / 2) * stem_c;
    for (const RnUnit& u : units) { max_act = std::max(max_act, u.out_elems()); max_act = std::max(max_act, u.in_elems()); }
    const size_t stem_hw = (size_t)(img_h / 2) * (img_w / 2);
    LRP_TRY(images.alloc(B * img_h * img_w * 3 * 4, total));
    LRP_TRY(stemA.alloc(B * stem_hw * 2 * RN_STEM_K * 4, total));
    LRP_TRY(a0.alloc(B * stem_hw * stem_c * 4, total));
    LRP_TRY(q_stem.alloc(B * stem_hw * stem_c * 4, total));
    LRP_TRY(pool_win.alloc(B * (stem_hw / 4) * stem_c, total));
    for (DevBuf* d : {&fa, &fb, &fc, &fz, &fsc, &fxs}) LRP_TRY(d->alloc(B * max_act * 4, total));
    LRP_TRY(act_max.alloc((units.size() + blocks.size()) * ACT_MAX_SLOTS * sizeof(unsigned), total));
    LRP_TRY(act_unscale.alloc(units.size() * sizeof(float), total));
    LRP_TRY(eslots.alloc((units.size() + blocks.size()) * B * ACT_MAX_SLOTS * sizeof(unsigned), total));
    LRP_TRY(eoscale.alloc(units.size() * B * sizeof(float), total));
    LRP_TRY(eunscale.alloc(units.size() * B * sizeof(float), total));
    LRP_TRY(fnorm.alloc(units.size() * 2 * sizeof(float), total));
    LRP_TRY(feat.alloc(B * (size_t)top_h * top_w * top_c * 4, total));
    const size_t max_tok = std::max(max_act, stem_hw * (size_t)std::max(RN_STEM_TCOLS, stem_c));
    for (DevBuf* d : {&r0, &r1, &r2, &r3, &r4, &r5}) LRP_TRY(d->alloc(NT * max_tok * 4, total));
    for (RnUnit& u : units) LRP_TRY(u.gate.alloc(B * u.out_elems() * 4, total));
    for (RnBlock& b : blocks) {
      LRP_TRY(b.t_in.alloc(B * (size_t)b.Hin * b.Win * b.cin * 4, total));
      if (b.stride == 2) LRP_TRY(b.t_sub.alloc(B * (size_t)b.H * b.W * b.cin * 4, total));
      LRP_TRY(b.GA.alloc(B * (size_t)b.H * b.W * 4 * b.f * 4, total));
      LRP_TRY(b.GS.alloc(B * (size_t)b.H * b.W * 4 * b.f * 4, total));
    }
    // staging of the weight setters (allocated here: lrp_set_weight_dev promises no allocation / stream synchronisation)
    size_t mx = 0, mxd = 0;
    for (const RnUnit& q : units) {
      mx = std::max(mx, (size_t)q.k * q.k * q.cin * q.cout);
      mxd = std::max(mxd, (size_t)conv_npad(2 * q.cout) * q.k * q.k * conv_cinp(q.cin));
    }
    LRP_TRY(raw_tmp.alloc(mx * 4, total));
    LRP_TRY(pack_tmp.alloc(mxd * 4, total));
    return LRP_OK;
  }
  ~ResNetEncoder() {
    if (ev_pack) (void)hipEventDestroy(ev_pack);
  }

  int find_unit(const std::string& nm) const {
    for (size_t i = 0; i < units.size(); ++i)
      if (units[i].name == nm) return (int)i;
    return -1;
  }

  // name = "<unit>_conv_W" | "_conv_b" | "_bn_gamma" | "_bn_beta" | "_bn_mean" | "_bn_var"; returns 1 if not ours.
  // `data` is a host array (lrp_set_weight) or already in HBM (lrp_set_weight_dev: RCCL broadcast), `kind` says which:
  // vectors are one copy, kernels are copied into the staging buffer and packed by device kernels — no device-to-host
  // copy, no allocation after a unit's first set, no stream synchronisation.
  // ONE staging pair for every unit (largest interleaved dual matrix / largest HWIO kernel): a call's packers read it
  // asynchronously on that call's stream, so the NEXT call — possibly on another stream: an RCCL stream, then a compute
  // stream — first makes its stream wait for `ev_pack`, recorded behind the previous call's last reader.
  DevBuf pack_tmp, raw_tmp;
  hipEvent_t ev_pack = nullptr;
  int set_weight(const std::string& nm, const float* data, hipMemcpyKind kind, int ndim, const int64_t* shape, int64_t* total,
                 hipStream_t st) {
    static const char* suf[6] = {"_conv_W", "_conv_b", "_bn_gamma", "_bn_beta", "_bn_mean", "_bn_var"};
    for (int s = 0; s < 6; ++s) {
      const std::string sf(suf[s]);
      if (nm.size() <= sf.size() || nm.compare(nm.size() - sf.size(), sf.size(), sf) != 0) continue;
      const int ui = find_unit(nm.substr(0, nm.size() - sf.size()));
      if (ui < 0) return 1;
      RnUnit& u = units[ui];
      if (s == 0) {
        if (ndim != 4 || shape[0] != u.k || shape[1] != u.k || shape[2] != u.cin || shape[3] != u.cout)
          return fail(LRP_ERR_INVALID, "%s: expected HWIO (%d,%d,%d,%d)", nm.c_str(), u.k, u.k, u.cin, u.cout);
        // own copy first: the packers run asynchronously, the caller's buffer need not outlive this call
        const size_t nW = (size_t)u.k * u.k * u.cin * u.cout;
        if (!ev_pack) LRP_HIP_CHECK(hipEventCreateWithFlags(&ev_pack, hipEventDisableTiming));
        else LRP_HIP_CHECK(hipStreamWaitEvent(st, ev_pack, 0));          // the previous unit's packers still read the staging pair
        LRP_HIP_CHECK(hipMemcpyAsync(raw_tmp.p, data, nW * 4, kind, st));
        LRP_TRY(pack_unit_dev(u, raw_tmp.as<float>(), st));
        LRP_HIP_CHECK(hipEventRecord(ev_pack, st));
      } else {
        if (ndim != 1 || shape[0] != u.cout) return fail(LRP_ERR_INVALID, "%s: expected (%d,)", nm.c_str(), u.cout);
        DevBuf* dst[6] = {nullptr, &u.bias, &u.gamma, &u.beta, &u.mean, &u.var};
        if (!dst[s]->p || dst[s]->bytes != (size_t)u.cout * 4) LRP_TRY(dst[s]->alloc((size_t)u.cout * 4, total));
        LRP_HIP_CHECK(hipMemcpyAsync(dst[s]->p, data, (size_t)u.cout * 4, kind, st));
      }
      u.have[s] = true;
      u.grad_ok = false;
      u.ab_packed = false;
      u.rule_packed = false;
      norms_ready = false;
      encoded = 0;                                       // caches belong to the old weights
      return LRP_OK;
    }
    return 1;
  }
  // `d` holds at least `floats` floats afterwards: allocated at its first use, grown (the handle's workspace counter corrected
  // for the buffer that goes) where a later caller needs more — the walk's scratch under the first two-chain rule — and left
  // alone otherwise.  A unit's matrices depend on its geometry alone, so for them "at least" and "exactly" are the same test:
  // they are allocated once, and a weight set again finds them.
  int reserve(DevBuf& d, size_t floats) {
    if (d.p && d.bytes >= floats * sizeof(float)) return LRP_OK;
    if (d.p && ws_total) *ws_total -= (int64_t)d.bytes;
    return d.alloc(floats * sizeof(float), ws_total);
  }
  // dst = the split8 form (bf16x3 operand) of the n floats at src
  void split_copy(const float* src, float* dst, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(n / 8)), dim3(256), 0, st, src, dst, n / 8);
  }
  int pack_unit_dev(RnUnit& u, const float* w_dev, hipStream_t st) {
    if (u.k == 7) {
      const int Np = conv_npad(u.cout), K = 2 * RN_STEM_K, Npb = conv_npad(RN_STEM_TCOLS), Kb = conv_cinp(u.cout);
      LRP_TRY(reserve(u.w_a, (size_t)Np * K)); LRP_TRY(reserve(u.w_z, (size_t)Np * K)); LRP_TRY(reserve(u.w_b, (size_t)Npb * Kb));
      hipLaunchKernelGGL(rn_pack_stem_dev_kernel, dim3(stream_grid((size_t)Np * K + (size_t)Npb * Kb)), dim3(256), 0, st, w_dev,
                         u.w_a.as<float>(), u.w_z.as<float>(), u.w_b.as<float>(), u.cout, Np, Npb, Kb);
      if (!(u.cout & 7)) {
        LRP_TRY(reserve(u.w_bs, (size_t)Npb * Kb));
        split_copy(u.w_b.as<float>(), u.w_bs.as<float>(), (size_t)Npb * Kb, st);
      }
      LRP_HIP_CHECK(hipGetLastError());
      return LRP_OK;
    }
    const int taps = u.k * u.k, CPi = conv_cinp(u.cin), CPo = conv_cinp(u.cout);
    const int Np = conv_npad(u.cout), Npb = conv_npad(u.cin);
    const size_t nf = (size_t)Np * taps * CPi, nb = (size_t)Npb * taps * CPo;
    auto pack = [&](float* dst, int bwd, int rows, int dual, int pos) {
      const size_t tot = (size_t)rows * taps * (bwd ? CPo : CPi);
      hipLaunchKernelGGL(pack_conv_dev_kernel, dim3(stream_grid(tot)), dim3(256), 0, st, w_dev, dst, bwd, u.cin, u.cout, bwd ? CPo : CPi,
                         rows, dual, pos, taps);
    };
    LRP_TRY(reserve(u.w_a, nf)); LRP_TRY(reserve(u.w_z, nf));
    pack(u.w_a.as<float>(), 0, Np, 0, 0);
    pack(u.w_z.as<float>(), 0, Np, 0, 1);                // inputs are post-ReLU: Z = conv(x, w+) + b
    if (!(u.cout & 3)) {
      const int Nd = conv_npad(2 * u.cout);
      const size_t nd = (size_t)Nd * taps * CPi;
      LRP_TRY(reserve(u.w_dual, nd));
      pack(u.w_dual.as<float>(), 0, Nd, 1, 0);
      if (!(u.cin & 7)) {
        u.dual_il = !(u.cout & 31) && Nd == 2 * u.cout;
        const float* src = u.w_dual.as<float>();
        if (u.dual_il) {                                  // rows in blocks of 32: [w | w+] of the same 32 channels
          pack(pack_tmp.as<float>(), 0, Nd, 2, 0);
          src = pack_tmp.as<float>();
        }
        LRP_TRY(make_f16_operand(f16_slots, src, nd, 0, 0, u.w_dual_h, u.wds, ws_total, st));
      }
    }
    LRP_TRY(reserve(u.w_b, nb)); LRP_TRY(reserve(u.w_bs, nb));
    pack(u.w_b.as<float>(), 1, Npb, 0, 1);
    split_copy(u.w_b.as<float>(), u.w_bs.as<float>(), nb, st);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }

  // ---- alpha-beta rule (lrp_set_cnn_rule; RR:274-322 with beta > 0) ----
  // Per conv + BN unit two denominators, Za = conv(x, w+) + b (the forward's Z) and Zi = conv(x, w-) + b, both with the full
  // bias, hence two gates Bn / safe(Za) and Bn / safe(Zi); the walk carries [S_a | S_i] as one tensor and every transposed conv is
  // ONE GEMM over both chains against [alpha w+ ; -beta w-] (explain_ab).  beta = 0 (the default) is the alpha1beta0 walk:
  // nothing here is allocated, launched or read, and what the (1, 0) walk reads is written by the same launches either way.
  // The handle's rule is a PAIR (lrp_set_resnet_rules): one record for the stem conv, one for every conv above it.
  // lrp_set_cnn_rule(alpha, beta) is the pair with that alpha-beta-with-bias record twice (one_rule()): the walk above, made by
  // the launches above.  Every other pair leaves the forward as it is and makes its gates behind it (rule_gates).
  struct Rule {
    int kind = LRP_RULE_ALPHA_BETA, bias = 1;
    float alpha = 1.f, beta = 0.f, eps = 0.f, low = 0.f, high = 0.f;
    int chains() const { return kind == LRP_RULE_ALPHA_BETA && beta > 0.f ? 2 : 1; }
    bool input_only() const { return kind == LRP_RULE_FLAT || kind == LRP_RULE_WSQUARE || kind == LRP_RULE_BOUNDED; }
    bool on_default_matrix() const { return (kind == LRP_RULE_ALPHA_BETA && beta == 0.f) || kind == LRP_RULE_BOUNDED; }   // w_b / w_bs
    bool same(const Rule& o) const {
      return kind == o.kind && bias == o.bias && alpha == o.alpha && beta == o.beta && eps == o.eps && low == o.low && high == o.high;
    }
  };
  Rule rule_stem, rule_units;
  const Rule& rule_of(const RnUnit& u) const { return u.k == 7 ? rule_stem : rule_units; }
  bool one_rule() const {
    return rule_stem.kind == LRP_RULE_ALPHA_BETA && rule_stem.bias && rule_stem.same(rule_units);
  }
  bool ab_on() const { return one_rule() && rule_units.beta > 0.f; }      // the second gates ride on the forward's own launches
  bool two_chains() const { return rule_stem.chains() == 2 || rule_units.chains() == 2; }
  bool has_eps() const { return rule_stem.kind == LRP_RULE_EPSILON || rule_units.kind == LRP_RULE_EPSILON; }
  DevBuf q_stem_i;
  DevBuf stem_dconst;      // the stem's constant denominator per channel (flat, w-square, bounded: rn_stem_rule_consts_kernel)
  // the dual-gate epilogue works on whole split8 groups of either chain (conv_plan: Cin % 16 == 0 over both chains)
  bool ab_supported() const {
    if (stem_c & 7) return false;
    for (const RnBlock& b : blocks)
      if (b.f & 7) return false;
    return true;
  }
  // both records are validated (engine.hip).  Every buffer appears, or grows, with the first pair that needs it, and stays (idle)
  // under a later pair that does not
  int set_rules(const Rule& rs, const Rule& ru) {
    if (rs.same(rule_stem) && ru.same(rule_units)) return LRP_OK;
    if ((rs.chains() == 2 || ru.chains() == 2) && !ab_supported())
      return fail(LRP_ERR_UNSUPPORTED, "alpha-beta with beta > 0 on a ResNet encoder needs a stem width and stack widths that are multiples of 8");
    const size_t B = max_images, NT = max_tokens;
    const size_t stem_hw = (size_t)(img_h / 2) * (img_w / 2);
    const bool on_fwd = rs.kind == LRP_RULE_ALPHA_BETA && rs.bias && rs.same(ru);      // one_rule() of the new pair
    for (RnUnit& u : units) {
      const Rule& r = u.k == 7 ? rs : ru;
      const int taps = u.k * u.k;
      if (r.chains() == 2) {
        if (u.k == 7) {                                  // (the stem's second gate is q_stem_i)
          LRP_TRY(reserve(u.w_n, (size_t)conv_npad(u.cout) * 2 * RN_STEM_K));
          const size_t nb = (size_t)conv_npad(RN_STEM_TCOLS) * conv_cinp(2 * u.cout);
          LRP_TRY(reserve(u.w_ab, nb)); LRP_TRY(reserve(u.w_abs, nb));
        } else {
          LRP_TRY(reserve(u.gate_i, B * u.out_elems()));
          LRP_TRY(reserve(u.w_n, (size_t)conv_npad(u.cout) * taps * conv_cinp(u.cin)));
          if (on_fwd && u.dual_il && u.w_dual_h.p) LRP_TRY(reserve(u.w_dualn_h, (size_t)conv_npad(2 * u.cout) * taps * conv_cinp(u.cin)));
          const size_t nb = (size_t)conv_npad(u.cin) * taps * conv_cinp(2 * u.cout);
          LRP_TRY(reserve(u.w_ab, nb)); LRP_TRY(reserve(u.w_abs, nb));
        }
      } else if (!r.on_default_matrix()) {
        const size_t nb = u.k == 7 ? (size_t)conv_npad(RN_STEM_TCOLS) * conv_cinp(u.cout) : (size_t)conv_npad(u.cin) * taps * conv_cinp(u.cout);
        LRP_TRY(reserve(u.w_r, nb));
        // (split8 serves the bf16x3 walk, which no epsilon kind takes: flat and w-square at the stem alone)
        if (r.kind != LRP_RULE_EPSILON && !(u.cout & 7)) LRP_TRY(reserve(u.w_rs, nb));
      }
    }
    if (ru.chains() == 2)
      for (RnBlock& b : blocks) {
        const size_t ne = B * (size_t)b.H * b.W * 4 * b.f;
        LRP_TRY(reserve(b.GA_i, ne));
        if (b.u0 >= 0) LRP_TRY(reserve(b.GS_i, ne));
      }
    if (rs.chains() == 2) LRP_TRY(reserve(q_stem_i, B * stem_hw * stem_c));
    if (rs.input_only()) LRP_TRY(reserve(stem_dconst, (size_t)stem_c));
    if (rs.chains() == 2 || ru.chains() == 2) {
      // the per-token scratch of the tensors that carry two chains (S3 / S0, S2, S1, the pool routing's output)
      size_t max_act = stem_hw * stem_c;
      for (const RnUnit& u : units) max_act = std::max(max_act, std::max(u.out_elems(), u.in_elems()));
      const size_t tok2 = std::max(2 * max_act, stem_hw * (size_t)RN_STEM_TCOLS);
      for (DevBuf* d : {&r1, &r2, &r3, &r5}) LRP_TRY(reserve(*d, NT * tok2));
    }
    rule_stem = rs; rule_units = ru;
    for (RnUnit& u : units) { u.ab_packed = false; u.rule_packed = false; }
    encoded = 0;                                         // the caches belong to the old pair
    return LRP_OK;
  }
  int set_rule(float alpha, float beta) {                // lrp_set_cnn_rule: the record with the bias, twice
    Rule r;
    r.alpha = alpha; r.beta = beta;
    return set_rules(r, r);
  }
  // the pair's matrices of every unit whose weights or rule changed since its last packing, from the resident forward matrix w_a
  int ensure_ab_weights(hipStream_t st) {
    for (RnUnit& u : units) {
      const Rule& r = rule_of(u);
      if (u.ab_packed || r.chains() != 2) continue;
      // a weight set after the rule may have changed which forward path the unit takes
      if (ab_on() && u.k != 7 && u.dual_il && u.w_dual_h.p)
        LRP_TRY(reserve(u.w_dualn_h, (size_t)conv_npad(2 * u.cout) * u.k * u.k * conv_cinp(u.cin)));
      if (u.k == 7) {
        const int Np = conv_npad(u.cout), Npb = conv_npad(RN_STEM_TCOLS), Kb2 = conv_cinp(2 * u.cout);
        const size_t nf = (size_t)Np * 2 * RN_STEM_K, nb = (size_t)Npb * Kb2;
        hipLaunchKernelGGL(rn_pack_stem_ab_kernel, dim3(stream_grid(nf + nb)), dim3(256), 0, st, u.w_a.as<float>(), u.w_n.as<float>(),
                           u.w_ab.as<float>(), u.cout, Np, Npb, Kb2, r.alpha, r.beta);
        split_copy(u.w_ab.as<float>(), u.w_abs.as<float>(), nb, st);
      } else {
        const int taps = u.k * u.k, CPi = conv_cinp(u.cin), CP2 = conv_cinp(2 * u.cout), rows = conv_npad(u.cin);
        const size_t nf = (size_t)conv_npad(u.cout) * taps * CPi, nb = (size_t)rows * taps * CP2;
        hipLaunchKernelGGL(rn_pack_neg_kernel, dim3(stream_grid(nf)), dim3(256), 0, st, u.w_a.as<float>(), u.w_n.as<float>(), nf);
        if (ab_on() && u.w_dualn_h.p) {
          const int Nd = conv_npad(2 * u.cout);
          hipLaunchKernelGGL(rn_pack_dual_neg_h_kernel, dim3(stream_grid((size_t)Nd * taps * CPi / 8)), dim3(256), 0, st, u.w_a.as<float>(),
                             u.w_dualn_h.as<float>(), taps * CPi, Nd, u.wds.as<float>());
        }
        hipLaunchKernelGGL(rn_pack_ab_kernel, dim3(stream_grid(nb)), dim3(256), 0, st, u.w_a.as<float>(), u.w_ab.as<float>(), taps, u.cin,
                           u.cout, CPi, CP2, rows, r.alpha, r.beta);
        split_copy(u.w_ab.as<float>(), u.w_abs.as<float>(), nb, st);
      }
      LRP_HIP_CHECK(hipGetLastError());
      u.ab_packed = true;
    }
    return LRP_OK;
  }
  // ... and the one-chain matrices of the records that do not walk on w_b (w_r / w_rs), and the stem's constant denominator
  int ensure_rule_weights(hipStream_t st) {
    for (RnUnit& u : units) {
      const Rule& r = rule_of(u);
      if (u.rule_packed) continue;
      if (u.k == 7 && r.input_only())
        hipLaunchKernelGGL(rn_stem_rule_consts_kernel, dim3((u.cout + 255) / 256), dim3(256), 0, st, u.w_a.as<float>(), stem_dconst.as<float>(),
                           u.cout, r.kind, r.low, r.high);
      if (r.chains() == 1 && !r.on_default_matrix()) {
        if (u.k == 7) {
          const int Npb = conv_npad(RN_STEM_TCOLS), Kb = conv_cinp(u.cout);
          const size_t nb = (size_t)Npb * Kb;
          hipLaunchKernelGGL(rn_pack_stem_rule_kernel, dim3(stream_grid(nb)), dim3(256), 0, st, u.w_a.as<float>(), u.w_r.as<float>(), u.cout,
                             Npb, Kb, r.kind);
          if (r.kind != LRP_RULE_EPSILON && u.w_rs.p) split_copy(u.w_r.as<float>(), u.w_rs.as<float>(), nb, st);
        } else {
          const int taps = u.k * u.k, CPi = conv_cinp(u.cin), CPo = conv_cinp(u.cout), rows = conv_npad(u.cin);
          const size_t nb = (size_t)rows * taps * CPo;
          hipLaunchKernelGGL(rn_pack_pq_kernel, dim3(stream_grid(nb)), dim3(256), 0, st, u.w_a.as<float>(), u.w_r.as<float>(), taps, u.cin,
                             u.cout, CPi, CPo, rows, 1.f, 1.f);       // (p, q) = (1, 1): the full w
        }
      }
      LRP_HIP_CHECK(hipGetLastError());
      u.rule_packed = true;
    }
    return LRP_OK;
  }
  // the inhibitor gate of a unit from c (what the forward's conv left in `c`) and one more conv for Zi (`cz`: the unit's forward
  // launch on fp32 operands); Zi goes through fz
  int unit_gate_inh(RnUnit& u, ConvArgs cz, const float* c, float* gate, int B, int relu, hipStream_t st) {
    cz.wpk = u.w_n.as<float>(); cz.out = fz.as<float>();
    LRP_HIP_CHECK(conv_launch(EPI_BIAS, cz, st));
    const size_t n = (size_t)B * u.out_elems();
    hipLaunchKernelGGL(rn_gate_inh_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, st, c, fz.as<float>(), u.gamma.as<float>(),
                       u.beta.as<float>(), u.mean.as<float>(), u.var.as<float>(), RN_BN_EPS, gate, n, u.cout, relu);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }
  int block_gates_inh(RnBlock& b, const float* sc, const float* y3, int B, hipStream_t st) {
    const size_t n = (size_t)B * b.H * b.W * 4 * b.f;
    hipLaunchKernelGGL(rn_block_gates_inh_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, st, sc, y3, units[b.u3].gate_i.as<float>(),
                       b.u0 >= 0 ? units[b.u0].gate_i.as<float>() : (const float*)nullptr, b.GA_i.as<float>(),
                       b.u0 >= 0 ? b.GS_i.as<float>() : (float*)nullptr, n);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }

  int check_ready() const {
    for (const RnUnit& u : units)
      for (int s = 0; s < 6; ++s)
        if (!u.have[s]) return fail(LRP_ERR_STATE, "ResNet weights of '%s' incomplete", u.name.c_str());
    return LRP_OK;
  }

  unsigned* unit_slots(int ui) { return act_max.as<unsigned>() + (size_t)ui * ACT_MAX_SLOTS; }
  unsigned* block_slots(size_t bi) { return act_max.as<unsigned>() + (units.size() + bi) * ACT_MAX_SLOTS; }

  // a unit's forward conv over x on fp32 operands and the unit's own weights: geometry (3x3: the image grid; 1x1: one row per
  // output pixel), bias, Cin / CinP.  The callers add the matrix, the outputs and what their operand format needs
  ConvArgs fwd_args(const RnUnit& u, const float* x, int B) const {
    ConvArgs ca{};
    ca.in = x; ca.bias = u.bias.as<float>(); ca.N = u.cout; ca.Cin = u.cin; ca.CinP = conv_cinp(u.cin);
    if (u.k == 3) { ca.NB = B; ca.H = u.Hout; ca.W = u.Wout; ca.taps = 9; }
    else { ca.NB = B * u.Hout * u.Wout; ca.H = 1; ca.W = 1; ca.taps = 1; }
    return ca;
  }
  // BatchNorm, ReLU and the unit's gate in the epilogue of a dual_il unit's conv: c and Z+ never go to memory (conv_args.h
  // ConvArgs::dual_gate = 2); act = relu(BN) or BN (nullptr with skip_out), the gate into u.gate
  static void bn_epilogue(ConvArgs& ca, const RnUnit& u, float* act) {
    ca.dual_il = 1; ca.dual_gate = 2; ca.bn_gamma = u.gamma.as<float>(); ca.bn_beta = u.beta.as<float>();
    ca.bn_mean = u.mean.as<float>(); ca.bn_var = u.var.as<float>(); ca.bn_eps = RN_BN_EPS; ca.bn_relu = u.relu ? 1 : 0;
    ca.out = act; ca.out2 = u.gate.as<float>();
  }
  // the inhibitor gate of a dual_il unit (beta > 0): the launch `ca` has just made again, [w | w-] in place of [w | w+] — same
  // operands, scales and epilogue — writing the gate alone: no activation, no pairs, no maxima
  int launch_inh_dual(const RnUnit& u, ConvArgs& ca, hipStream_t st) {
    ca.wpk = u.w_dualn_h.as<float>(); ca.out2 = u.gate_i.as<float>(); ca.skip_out = 1;
    ca.pairs_out = nullptr; ca.pairs_scale = nullptr; ca.act_max_out = nullptr;
    LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, ca, st, PREC_F16X2));
    return LRP_OK;
  }

  // conv + BN unit forward: x [B][Hin][Win][cin] -> act (relu(BN) or BN) and the unit's gate.
  // slots_in: maxima of x (fp16-pair forward: the power of two x is scaled by); slots_out: where max|act| is collected
  // (nullptr: nobody convolves this output)
  int unit_forward(RnUnit& u, const float* x, int B, float* act, hipStream_t st, const unsigned* slots_in = nullptr,
                   unsigned* slots_out = nullptr, unsigned char* mask = nullptr) {
    const float* xin = x;
    if (u.k == 1 && u.stride == 2) {
      const size_t n = (size_t)B * u.Hout * u.Wout * u.cin;
      hipLaunchKernelGGL(rn_subsample2_kernel, dim3(stream_grid(n)), dim3(256), 0, st, x, fsc.as<float>(), B, u.Hin, u.Win, u.cin);
      LRP_HIP_CHECK(hipGetLastError());
      xin = fsc.as<float>();
    }
    ConvArgs ca = fwd_args(u, xin, B);
    const int ui = (int)(&u - units.data());
    if (u.w_dual_h.p && slots_in && prec == PREC_BF16X3) {
      // the same single pass on the fp16 MFMA: x and (w | w+) as fp16 pairs, the product in three MFMAs with blocked
      // fp32 accumulation (conv_args.h PREC_F16X2) — fp32-grade, ~2.5x the fp32 matrix rate
      const size_t n8 = (size_t)B * u.Hout * u.Wout * u.cin / 8;
      hipLaunchKernelGGL(split_h_scaled_kernel, dim3(stream_grid(n8)), dim3(256), 0, st, xin, fxs.as<float>(), n8, slots_in,
                         act_unscale.as<float>() + ui, u.wds.as<float>());
      LRP_HIP_CHECK(hipGetLastError());
      ca.in = fxs.as<float>(); ca.wpk = u.w_dual_h.as<float>(); ca.N = 2 * u.cout; ca.split = u.cout; ca.dual_norelu = 1;
      ca.out = fc.as<float>(); ca.out2 = fz.as<float>(); ca.in_unscale = act_unscale.as<float>() + ui;
      if (u.dual_il) {
        bn_epilogue(ca, u, act);
        ca.act_max_out = slots_out;
        LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, ca, st, PREC_F16X2));
        if (ab_on()) LRP_TRY(launch_inh_dual(u, ca, st));
        return LRP_OK;
      }
      LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, ca, st, PREC_F16X2));
    } else if (u.w_dual.p) {
      // c = conv(x, w) + b and Z = conv(x, w+) + b in ONE pass over x: the A tile is staged once for both
      ca.wpk = u.w_dual.as<float>(); ca.N = 2 * u.cout; ca.split = u.cout; ca.dual_norelu = 1;
      ca.out = fc.as<float>(); ca.out2 = fz.as<float>();
      LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, ca, st));
    } else {
      ca.wpk = u.w_a.as<float>(); ca.out = fc.as<float>();
      LRP_HIP_CHECK(conv_launch(EPI_BIAS, ca, st));
      ca.wpk = u.w_z.as<float>(); ca.out = fz.as<float>();
      LRP_HIP_CHECK(conv_launch(EPI_BIAS, ca, st));
    }
    const size_t n = (size_t)B * u.out_elems();
    hipLaunchKernelGGL(rn_bn_unit_kernel, dim3(stream_grid(n)), dim3(256), 0, st, fc.as<float>(), fz.as<float>(),
                       u.gamma.as<float>(), u.beta.as<float>(), u.mean.as<float>(), u.var.as<float>(), RN_BN_EPS, act,
                       u.gate.as<float>(), (float*)nullptr, n, u.cout, u.relu ? 1 : 0, slots_out, mask);
    LRP_HIP_CHECK(hipGetLastError());
    if (ab_on()) LRP_TRY(unit_gate_inh(u, fwd_args(u, xin, B), fc.as<float>(), u.gate_i.as<float>(), B, u.relu ? 1 : 0, st));
    return LRP_OK;
  }

  // ---- round 4: no pass between two convs (kernels and the bounds behind the scales: resnet_kernels.h) ----
  unsigned* eslots_unit(int ui) { return eslots.as<unsigned>() + (size_t)ui * max_images * ACT_MAX_SLOTS; }
  unsigned* eslots_block(size_t bi) { return eslots.as<unsigned>() + (units.size() + bi) * max_images * ACT_MAX_SLOTS; }
  float* eoscale_unit(int ui) { return eoscale.as<float>() + (size_t)ui * max_images; }
  float* eunscale_unit(int ui) { return eunscale.as<float>() + (size_t)ui * max_images; }
  float* fnorm_unit(int ui) { return fnorm.as<float>() + (size_t)ui * 2; }
  static dim3 img_grid(size_t per_img_items, int B) {
    size_t gx = (per_img_items + 255) / 256, cap = (size_t)std::max(1, 256 * 8 / B);
    return dim3((unsigned)std::max<size_t>(1, std::min(gx, cap)), (unsigned)B);
  }
  // the whole network on the pair-emitting path: fp16-pair forward, every unit behind the stem with interleaved dual rows
  // (cout % 32 == 0) and whole split8 groups on its input (cin % 8 == 0).  ResNet-50/101/152 qualify; LRP_FWD_EMIT=0 = round 3's path
  bool emit_ok() const {
    if (prec != PREC_BF16X3 || !sw().fwd_emit || (stem_c & 7)) return false;
    for (size_t i = 1; i < units.size(); ++i)
      if (!units[i].w_dual_h.p || !units[i].dual_il || (units[i].cin & 7)) return false;
    return true;
  }
  int unit_norms(hipStream_t st) {
    LRP_HIP_CHECK(hipMemsetAsync(fnorm.p, 0, fnorm.bytes, st));
    for (size_t i = 1; i < units.size(); ++i) {
      const RnUnit& u = units[i];
      hipLaunchKernelGGL(rn_unit_norm_kernel, dim3(u.cout), dim3(256), 0, st, u.w_a.as<float>(), u.k * u.k * conv_cinp(u.cin),
                         u.bias.as<float>(), u.gamma.as<float>(), u.beta.as<float>(), u.mean.as<float>(), u.var.as<float>(),
                         RN_BN_EPS, fnorm_unit((int)i));
    }
    LRP_HIP_CHECK(hipGetLastError());
    norms_ready = true;
    return LRP_OK;
  }
  // conv + BN unit on pairs: x (pairs, scaled per image) -> gate, max-slots and EITHER the activation as the next conv's pairs
  // (pairs_out: relu units inside a block; fp32 activation not written) OR the fp32 pre-Add tensor `act`
  int unit_forward_emit(RnUnit& u, const float* xpairs, int B, float* act, float* pairs_out, hipStream_t st) {
    const int ui = (int)(&u - units.data());
    ConvArgs ca = fwd_args(u, xpairs, B);
    ca.wpk = u.w_dual_h.as<float>(); ca.N = 2 * u.cout; ca.split = u.cout; ca.dual_norelu = 1;
    ca.in_unscale = eunscale_unit(ui);
    bn_epilogue(ca, u, act);
    ca.act_max_out = pairs_out ? (unsigned*)nullptr : eslots_unit(ui);      // measured maxima: the block end's two summands only
    ca.scale_per_img = 1; ca.img_rows = u.Hout * u.Wout; ca.n_imgs = B;
    if (pairs_out) { ca.pairs_out = pairs_out; ca.pairs_scale = eoscale_unit(ui); ca.skip_out = 1; }
    LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, ca, st, PREC_F16X2));
    if (ab_on()) LRP_TRY(launch_inh_dual(u, ca, st));
    return LRP_OK;
  }
  // the stem's forward up to its BatchNorm, for both paths: im2col -> two 1-tap GEMMs on the fp32 MFMA, c (exact) into fa and Z
  // (both sign branches) into fz.  cz: the Z launch, which unit_gate_inh runs once more against w_n under beta > 0
  ConvArgs stem_fwd_args(int B) const {                  // a 1-tap GEMM over the im2col rows in stemA
    const RnUnit& s = units[0];
    ConvArgs cz{};
    cz.in = stemA.as<float>(); cz.NB = B * s.Hout * s.Wout; cz.H = 1; cz.W = 1; cz.Cin = 2 * RN_STEM_K; cz.CinP = 2 * RN_STEM_K;
    cz.taps = 1; cz.N = s.cout; cz.bias = s.bias.as<float>();
    return cz;
  }
  int stem_forward(int B, ConvArgs& cz, hipStream_t st) {
    const RnUnit& s = units[0];
    const size_t tot = (size_t)B * s.Hout * s.Wout * 2 * RN_STEM_K;
    hipLaunchKernelGGL(rn_stem_im2col_kernel, dim3(stream_grid(tot)), dim3(256), 0, st, images.as<float>(),
                       stemA.as<float>(), B, img_h, img_w);
    LRP_HIP_CHECK(hipGetLastError());
    cz = stem_fwd_args(B);
    cz.wpk = s.w_a.as<float>(); cz.out = fa.as<float>();
    LRP_HIP_CHECK(conv_launch(EPI_BIAS, cz, st));
    cz.wpk = s.w_z.as<float>(); cz.out = fz.as<float>();
    LRP_HIP_CHECK(conv_launch(EPI_BIAS, cz, st));
    return LRP_OK;
  }
  int encode_emit(int B, hipStream_t st) {
    if (!norms_ready) LRP_TRY(unit_norms(st));
    LRP_HIP_CHECK(hipMemsetAsync(eslots.p, 0, eslots.bytes, st));
    RnUnit& s = units[0];
    auto scales_of = [&](const RnBlock& rb) {             // what the producer of rb's input derives for rb (resnet_kernels.h)
      RnBlockScales S{};
      S.norm1 = fnorm_unit(rb.u1); S.norm2 = fnorm_unit(rb.u2);
      S.wsc1 = units[rb.u1].wds.as<float>(); S.wsc2 = units[rb.u2].wds.as<float>(); S.wsc3 = units[rb.u3].wds.as<float>();
      S.wsc0 = rb.u0 >= 0 ? units[rb.u0].wds.as<float>() : (const float*)nullptr;
      S.osc_t = eoscale_unit(rb.u3);                     // (slot of a tensor that is never written as pairs itself)
      S.osc1 = eoscale_unit(rb.u1); S.osc2 = eoscale_unit(rb.u2);
      S.us1 = eunscale_unit(rb.u1); S.us2 = eunscale_unit(rb.u2); S.us3 = eunscale_unit(rb.u3);
      S.us0 = rb.u0 >= 0 ? eunscale_unit(rb.u0) : (float*)nullptr;
      return S;
    };
    float* tp = fc.as<float>();                          // the block input as pairs (fc / fsc alternate)
    float* tp_other = fsc.as<float>();
    {  // stem: im2col -> two 1-tap GEMMs (fp32 MFMA) -> BN + relu + gate -> pool (+ pairs of the first block's input)
      ConvArgs cz;
      LRP_TRY(stem_forward(B, cz, st));
      const size_t per = s.out_elems();
      hipLaunchKernelGGL(rn_bn_unit_img_kernel, img_grid(per, B), dim3(256), 0, st, fa.as<float>(), fz.as<float>(),
                         s.gamma.as<float>(), s.beta.as<float>(), s.mean.as<float>(), s.var.as<float>(), RN_BN_EPS,
                         a0.as<float>(), s.gate.as<float>(), q_stem.as<float>(), per, s.cout, 1, eslots_unit(0));
      hipLaunchKernelGGL(rn_pool3_pairs_kernel, img_grid(per / 4 / 8, B), dim3(256), 0, st, a0.as<float>(), blocks[0].t_in.as<float>(),
                         pool_win.as<unsigned char>(), tp, eslots_unit(0), scales_of(blocks[0]), s.Hout, s.Wout, s.cout);
      LRP_HIP_CHECK(hipGetLastError());
      if (ab_on()) LRP_TRY(unit_gate_inh(s, cz, fa.as<float>(), q_stem_i.as<float>(), B, 0, st));
    }
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
      RnBlock& b = blocks[bi];
      const float* t = b.t_in.as<float>();
      const unsigned* ts = bi == 0 ? eslots_unit(0) : eslots_block(bi - 1);      // per-image maxima of the block input
      const float* tin = tp;
      if (b.stride == 2) {
        // the walk multiplies with the fp32 sub-sampled input; the strided 1x1 convs read the same gather of the pairs
        // (a pixel's pairs are as many bytes as its fp32 row)
        const size_t n = (size_t)B * b.H * b.W * b.cin;
        hipLaunchKernelGGL(rn_subsample2_kernel, dim3(stream_grid(n)), dim3(256), 0, st, t, b.t_sub.as<float>(), B, b.Hin, b.Win, b.cin);
        hipLaunchKernelGGL(rn_subsample2_kernel, dim3(stream_grid(n)), dim3(256), 0, st, tp, fxs.as<float>(), B, b.Hin, b.Win, b.cin);
        LRP_HIP_CHECK(hipGetLastError());
        tin = fxs.as<float>();
      }
      RnUnit &u1 = units[b.u1], &u2 = units[b.u2], &u3 = units[b.u3];
      const float* sc = t;
      const unsigned* sc_slots = ts;
      if (b.u0 >= 0) {                                   // (first: it reads the gathered pairs, which unit 2 overwrites)
        LRP_TRY(unit_forward_emit(units[b.u0], tin, B, fb.as<float>(), nullptr, st));                   // fb = y0
        sc = fb.as<float>();
        sc_slots = eslots_unit(b.u0);
      }
      LRP_TRY(unit_forward_emit(u1, tin, B, nullptr, fz.as<float>(), st));                              // fz = pairs(a1)
      LRP_TRY(unit_forward_emit(u2, fz.as<float>(), B, nullptr, fxs.as<float>(), st));                  // fxs = pairs(a2)
      LRP_TRY(unit_forward_emit(u3, fxs.as<float>(), B, fa.as<float>(), nullptr, st));                  // fa = y3
      const bool last = bi + 1 == blocks.size();
      float* o = last ? feat.as<float>() : blocks[bi + 1].t_in.as<float>();
      const size_t per8 = (size_t)b.H * b.W * 4 * b.f / 8;
      hipLaunchKernelGGL(rn_block_out_pairs_kernel, img_grid(per8, B), dim3(256), 0, st, sc, fa.as<float>(), u3.gate.as<float>(),
                         b.u0 >= 0 ? units[b.u0].gate.as<float>() : (const float*)nullptr, o, b.GA.as<float>(), b.GS.as<float>(), per8,
                         last ? (unsigned*)nullptr : eslots_block(bi), last ? (float*)nullptr : tp_other, eslots_unit(b.u3), sc_slots,
                         last ? RnBlockScales{} : scales_of(blocks[bi + 1]));
      LRP_HIP_CHECK(hipGetLastError());
      if (ab_on()) LRP_TRY(block_gates_inh(b, sc, fa.as<float>(), B, st));
      std::swap(tp, tp_other);
    }
    return LRP_OK;
  }

  // the ReLU masks of the gradient walks (allocated by the first LRP_PREC_FP32 encode: other modes never pay for them)
  int alloc_masks() {
    const size_t B = max_images;
    for (RnBlock& b : blocks) {
      for (int ui : {b.u1, b.u2})
        if (!units[ui].mask.p) LRP_TRY(units[ui].mask.alloc(B * units[ui].out_elems(), ws_total));
      if (!b.omask.p) LRP_TRY(b.omask.alloc(B * (size_t)b.H * b.W * 4 * b.f, ws_total));
    }
    return LRP_OK;
  }

  int encode(const float* images_dev, int B, hipStream_t st) {
    if (B < 1 || B > max_images) return fail(LRP_ERR_INVALID, "B=%d outside [1,%d]", B, max_images);
    LRP_TRY(check_ready());
    if (two_chains()) LRP_TRY(ensure_ab_weights(st));
    if (!one_rule()) LRP_TRY(ensure_rule_weights(st));
    LRP_HIP_CHECK(hipMemcpyAsync(images.p, images_dev, (size_t)B * img_h * img_w * 3 * 4, hipMemcpyDeviceToDevice, st));
    masks_ok = false;
    if (emit_ok()) LRP_TRY(encode_emit(B, st));
    else LRP_TRY(encode_fp32_acts(B, st));               // (sets masks_ok in LRP_PREC_FP32 mode)
    if (!one_rule()) LRP_TRY(rule_gates(B, st));         // the pair's gates, behind the unchanged forward
    encoded = B;
    features_only = false;
    return LRP_OK;
  }
  // the forward with an fp32 activation between every two convs: exact fp32 (LRP_PREC_FP32, widths that are no multiples of 8)
  // or fp16 pairs made per unit from that activation (bf16x3 with LRP_FWD_EMIT=0, or a unit that emit_ok refuses)
  int encode_fp32_acts(int B, hipStream_t st) {
    LRP_HIP_CHECK(hipMemsetAsync(act_max.p, 0, act_max.bytes, st));
    const bool rec = prec == PREC_FP32;                  // record the ReLU masks (the gradient walks exist in this mode only)
    if (rec) LRP_TRY(alloc_masks());
    auto mask_of = [&](RnUnit& u) { return rec ? u.mask.as<unsigned char>() : (unsigned char*)nullptr; };
    RnUnit& s = units[0];
    {  // stem: im2col -> two 1-tap GEMMs (c exact / Z with both sign branches) -> BN + relu + gate (fa is free until block 0's unit 1)
      ConvArgs cz;
      LRP_TRY(stem_forward(B, cz, st));
      const size_t n = (size_t)B * s.out_elems();
      hipLaunchKernelGGL(rn_bn_unit_kernel, dim3(stream_grid(n)), dim3(256), 0, st, fa.as<float>(), fz.as<float>(),
                         s.gamma.as<float>(), s.beta.as<float>(), s.mean.as<float>(), s.var.as<float>(), RN_BN_EPS,
                         a0.as<float>(), s.gate.as<float>(), q_stem.as<float>(), n, s.cout, 1, unit_slots(0), (unsigned char*)nullptr);
      LRP_HIP_CHECK(hipGetLastError());
      const size_t np = (size_t)B * (s.Hout / 2) * (s.Wout / 2) * s.cout;
      hipLaunchKernelGGL(rn_pool3_kernel, dim3(stream_grid(np)), dim3(256), 0, st, a0.as<float>(), blocks[0].t_in.as<float>(),
                         pool_win.as<unsigned char>(), B, s.Hout, s.Wout, s.cout);
      LRP_HIP_CHECK(hipGetLastError());
      if (ab_on()) LRP_TRY(unit_gate_inh(s, cz, fa.as<float>(), q_stem_i.as<float>(), B, 0, st));
    }
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
      RnBlock& b = blocks[bi];
      const float* t = b.t_in.as<float>();
      // maxima of the block input: the pooled stem activation (bounded by the stem's) or the previous block's output
      const unsigned* ts = bi == 0 ? unit_slots(0) : block_slots(bi - 1);
      if (b.stride == 2) {
        const size_t n = (size_t)B * b.H * b.W * b.cin;
        hipLaunchKernelGGL(rn_subsample2_kernel, dim3(stream_grid(n)), dim3(256), 0, st, t, b.t_sub.as<float>(), B, b.Hin,
                           b.Win, b.cin);
        LRP_HIP_CHECK(hipGetLastError());
      }
      // main path: fa <- a1, fb <- a2, fa <- y3 ; shortcut: fsc2 (= r0 scratch is per-token; use GS buffer as temp) ...
      LRP_TRY(unit_forward(units[b.u1], t, B, fa.as<float>(), st, ts, unit_slots(b.u1), mask_of(units[b.u1])));
      LRP_TRY(unit_forward(units[b.u2], fa.as<float>(), B, fb.as<float>(), st, unit_slots(b.u1), unit_slots(b.u2), mask_of(units[b.u2])));
      LRP_TRY(unit_forward(units[b.u3], fb.as<float>(), B, fa.as<float>(), st, unit_slots(b.u2)));        // fa = y3
      const float* sc = t;
      if (b.u0 >= 0) {
        LRP_TRY(unit_forward(units[b.u0], t, B, fb.as<float>(), st, ts));               // fb = y0
        sc = fb.as<float>();
      }
      const bool last = bi + 1 == blocks.size();
      float* o = last ? feat.as<float>() : blocks[bi + 1].t_in.as<float>();
      const size_t n = (size_t)B * b.H * b.W * 4 * b.f;
      hipLaunchKernelGGL(rn_block_out_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, st, sc, fa.as<float>(),
                         units[b.u3].gate.as<float>(), b.u0 >= 0 ? units[b.u0].gate.as<float>() : (const float*)nullptr, o,
                         b.GA.as<float>(), b.GS.as<float>(), n, last ? (unsigned*)nullptr : block_slots(bi),
                         rec ? b.omask.as<unsigned char>() : (unsigned char*)nullptr);
      LRP_HIP_CHECK(hipGetLastError());
      if (ab_on()) LRP_TRY(block_gates_inh(b, sc, fa.as<float>(), B, st));
    }
    masks_ok = rec;
    return LRP_OK;
  }

  // ---- the gates of a rule pair that is not the one-rule entry's (set_rules) ----
  // Behind the forward of either path, which is left exactly as it is (features, the default gates and every cache of the gradient
  // walks), the gates the walk reads are brought under the pair's denominators: the units' gate (and gate_i), the blocks' GA and a
  // projection's GS (and GA_i / GS_i), the stem's q_stem (and q_stem_i).  What the forward kept suffices as input: the stem's im2col
  // rows and every block input t_in / t_sub in fp32.  Per unit c = conv(x, w) + b, Za and (beta > 0) Zi are fp32 launches of the
  // unit's conv (EPI_BIAS: the dual_il units of the forward never write c or Z+), then ONE kernel per gate.
  // Above the stem a gate is the FORWARD's gate times safe(Za) / D — the forward's denominator over the rule's, BatchNorm's factor
  // untouched — never Bn / D made anew: the forward's gates, GA and GS are consistent with the block inputs it wrote (o = sc + y3,
  // fA + fS = 1, y cancelling in y Bn), and where sc + y3 or y is small a y3 in another arithmetic (the fp16-pair forward against
  // this pass's fp32) breaks that by O(y3 / o) rounding errors; the ratio of two denominators is well conditioned.  So GA takes
  // unit 3's ratio, a projection's GS unit 0's, an identity block's GS stays.  The stem's c is the forward's own launch again, bit
  // for bit: its gate is made directly.  The forward's scratch is free by now: fc = c, fz = Za, fxs = Zi, fa = a1, fb = a2.
  int rule_gate(const RnUnit& u, const Rule& r, const float* Z, const float* src, float* act, float* gate, int den, int B, int relu,
                hipStream_t st) {
    const size_t n = (size_t)B * u.out_elems();
    hipLaunchKernelGGL(rn_rule_gate_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, st, fc.as<float>(), Z, fz.as<float>(), u.bias.as<float>(),
                       stem_dconst.as<float>(), u.gamma.as<float>(), u.beta.as<float>(), u.mean.as<float>(), u.var.as<float>(), RN_BN_EPS, src,
                       act, gate, n, u.cout, relu, den, r.bias ? 0 : 1, r.eps);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }
  // the stem: its forward's launches again (stem_fwd_args), q_stem (and q_stem_i) = Bn / D
  int rule_stem_gates(int B, hipStream_t st) {
    const RnUnit& s = units[0];
    const Rule& r = rule_stem;
    ConvArgs ca = stem_fwd_args(B);
    ca.wpk = s.w_a.as<float>(); ca.out = fc.as<float>();
    LRP_HIP_CHECK(conv_launch(EPI_BIAS, ca, st));
    if (r.kind != LRP_RULE_ALPHA_BETA) {
      const int den = r.kind == LRP_RULE_EPSILON ? 1 : r.kind == LRP_RULE_BOUNDED ? 3 : 2;
      return rule_gate(s, r, nullptr, nullptr, nullptr, q_stem.as<float>(), den, B, 0, st);
    }
    ca.wpk = s.w_z.as<float>(); ca.out = fz.as<float>();
    LRP_HIP_CHECK(conv_launch(EPI_BIAS, ca, st));
    LRP_TRY(rule_gate(s, r, fz.as<float>(), nullptr, nullptr, q_stem.as<float>(), 0, B, 0, st));
    if (r.beta > 0.f) {
      ca.wpk = s.w_n.as<float>(); ca.out = fxs.as<float>();
      LRP_HIP_CHECK(conv_launch(EPI_BIAS, ca, st));
      LRP_TRY(rule_gate(s, r, fxs.as<float>(), nullptr, nullptr, q_stem_i.as<float>(), 0, B, 0, st));
    }
    return LRP_OK;
  }
  // one unit above the stem: `ca` is its forward launch on fp32 operands (fwd_args).  g: the forward's tensor that carries the
  // unit's denominator (gate of a relu unit, GA / GS of a pre-Add unit), scaled in place; g_i (beta > 0): where the inhibitor's
  // goes, made from g first.  act = relu(BN(c)), the next unit's input (nullptr: not wanted)
  int rule_unit(const RnUnit& u, const Rule& r, ConvArgs ca, float* act, float* g, float* g_i, int B, hipStream_t st) {
    ca.wpk = u.w_a.as<float>(); ca.out = fc.as<float>();
    LRP_HIP_CHECK(conv_launch(EPI_BIAS, ca, st));
    ca.wpk = u.w_z.as<float>(); ca.out = fz.as<float>();
    LRP_HIP_CHECK(conv_launch(EPI_BIAS, ca, st));
    if (r.chains() == 2) {
      ca.wpk = u.w_n.as<float>(); ca.out = fxs.as<float>();
      LRP_HIP_CHECK(conv_launch(EPI_BIAS, ca, st));
      LRP_TRY(rule_gate(u, r, fxs.as<float>(), g, act, g_i, 0, B, 1, st));
      act = nullptr;
      if (r.bias) return LRP_OK;                         // (the activator's gate is the forward's)
    }
    return rule_gate(u, r, fz.as<float>(), g, act, g, r.kind == LRP_RULE_EPSILON ? 1 : 0, B, 1, st);
  }
  int rule_gates(int B, hipStream_t st) {
    const Rule &rs = rule_stem, &ru = rule_units;
    if (!(rs.kind == LRP_RULE_ALPHA_BETA && rs.bias && rs.beta == 0.f)) LRP_TRY(rule_stem_gates(B, st));      // (that record's q_stem is the forward's)
    if (ru.kind == LRP_RULE_ALPHA_BETA && ru.bias && ru.beta == 0.f) return LRP_OK;      // (... and so are the units' gates)
    for (RnBlock& b : blocks) {
      RnUnit &u1 = units[b.u1], &u2 = units[b.u2], &u3 = units[b.u3];
      const float* tin = b.stride == 2 ? b.t_sub.as<float>() : b.t_in.as<float>();
      if (b.u0 >= 0) LRP_TRY(rule_unit(units[b.u0], ru, fwd_args(units[b.u0], tin, B), nullptr, b.GS.as<float>(), b.GS_i.as<float>(), B, st));
      LRP_TRY(rule_unit(u1, ru, fwd_args(u1, tin, B), fa.as<float>(), u1.gate.as<float>(), u1.gate_i.as<float>(), B, st));            // a1
      LRP_TRY(rule_unit(u2, ru, fwd_args(u2, fa.as<float>(), B), fb.as<float>(), u2.gate.as<float>(), u2.gate_i.as<float>(), B, st)); // a2
      LRP_TRY(rule_unit(u3, ru, fwd_args(u3, fb.as<float>(), B), nullptr, b.GA.as<float>(), b.GA_i.as<float>(), B, st));
    }
    return LRP_OK;
  }

  // the transposed conv through unit u, every walk's: S [n][Hout][Wout][chains * cout] -> out [n][Hout][Wout][cin].  The callers
  // add the matrix (w_b / w_bs, w_ab / w_abs over two chains, w_g), the gates and the epilogue
  static ConvArgs bwd_args(const RnUnit& u, int n, const int* row2img, const float* S, float* out, int chains = 1) {
    ConvArgs ca{};
    ca.in = S; ca.row2img = row2img; ca.out = out; ca.N = u.cin;
    ca.Cin = chains * u.cout; ca.CinP = conv_cinp(chains * u.cout); ca.NB = n; ca.H = u.Hout; ca.W = u.Wout; ca.taps = u.k == 3 ? 9 : 1;
    return ca;
  }
  // what the profiler books on it per chain: 2 n H W k^2 cout cin
  static double bwd_flop(const RnUnit& u, int n) { return 2.0 * n * u.Hout * u.Wout * (double)(u.k == 3 ? 9 : 1) * u.cout * u.cin; }

  // conv-LRP step through one unit: S [n][Hout][Wout][cout] -> out [n][Hout'][..][cin] = convT(S, w+) * aux[img]
  // split: S is in split8 form and the conv runs as bf16x3; plain_out: the result feeds an element-wise kernel (fp32)
  // instead of the next conv of the chain (split8)
  struct BlockTail {                // optional: residual join and the next block's chain head, fused into the epilogue
    const float* join = nullptr; const float* join_gate = nullptr; const float* gate2 = nullptr; float* out2 = nullptr;
  };
  int unit_backward(const RnUnit& u, int n, const int* row2img, const float* S, const float* aux, float* out, hipStream_t st,
                    bool split = false, bool plain_out = true, const BlockTail* tail = nullptr) {
    ConvArgs ca = bwd_args(u, n, row2img, S, out);
    if (tail) { ca.join = tail->join; ca.join_gate = tail->join_gate; ca.gate2 = tail->gate2; ca.out2s = tail->out2; }
    const bool own = !rule_units.on_default_matrix();    // (an epsilon kind: the full w, exact fp32 only)
    ca.wpk = own ? u.w_r.as<float>() : split ? u.w_bs.as<float>() : u.w_b.as<float>(); ca.aux = aux; ca.out_plain = plain_out ? 1 : 0;
    prof.begin(st);
    LRP_HIP_CHECK(conv_launch(EPI_MUL, ca, st, split ? PREC_BF16X3 : PREC_FP32));
    prof.end(st, bwd_flop(u, n));
    return LRP_OK;
  }

  int explain(int n, const int* row2img, const float* R_feat_dev, float* R_img_dev, hipStream_t st, int walk = LRP_WALK_LRP) {
    if (n < 1 || n > max_tokens) return fail(LRP_ERR_INVALID, "n=%d outside [1,%d]", n, max_tokens);
    if (encoded < 1 || features_only) return fail(LRP_ERR_STATE, "lrp_encode_images must run before the CNN explain");
    if (walk != LRP_WALK_LRP) return explain_grad(n, row2img, R_feat_dev, R_img_dev, st, walk);
    // epsilon kinds are exact-fp32 only (their gate is a step in the activation for small eps, and a ReLU decision
    // the fp16-pair forward takes differently moves the map by O(1))
    if (has_eps() && prec != PREC_FP32)
      return fail(LRP_ERR_UNSUPPORTED, "a rule pair with an epsilon kind runs in LRP_PREC_FP32 only: set it with lrp_set_precision "
                                       "and call lrp_encode_images again");
    if (rule_units.chains() == 2) {                      // every launch is asked about before the first runs
      LRP_TRY(explain_ab(n, row2img, R_feat_dev, R_img_dev, st, true));
      return explain_ab(n, row2img, R_feat_dev, R_img_dev, st, false);
    }
    if (!one_rule()) LRP_TRY(stem_end(nullptr, n, row2img, R_img_dev, st, true));      // (the convs above are the default walk's launches)
    const float* Ro = R_feat_dev;          // relevance at the current block's output
    float* cur = r0.as<float>();           // where the next R_t is written (ping-pong r0 / r4)
    float* other = r4.as<float>();
    float* s3 = r1.as<float>();            // S3 = R_o * GA of the block being walked (r1 / r5 alternate)
    float* s3_other = r5.as<float>();
    bool have_s3 = false;                  // already written by the previous block's fused epilogue
    auto block_split = [&](const RnBlock& bb) {
      bool v = prec == PREC_BF16X3;
      for (int ui : {bb.u0, bb.u1, bb.u2, bb.u3})
        if (ui >= 0 && ((units[ui].cin | units[ui].cout) & 7)) v = false;
      return v;
    };
    for (int bi = (int)blocks.size() - 1; bi >= 0; --bi) {
      const RnBlock& b = blocks[bi];
      const size_t per_o = (size_t)b.H * b.W * 4 * b.f;
      // bf16x3 mode: the convs of the main branch and of the projection in split8 form; the products that enter a chain are
      // written split, what leaves it for the join is plain fp32
      const bool sp = block_split(b);                    // split8 groups need channel counts % 8 == 0: exact fp32 otherwise
      auto head = [&](const float* G, float* dst) -> int {     // a chain's head: dst = R_o * G
        if (sp)
          hipLaunchKernelGGL(rn_mul_gate_split_kernel, dim3(stream_grid((size_t)n * per_o / 8)), dim3(256), 0, st, Ro, G, row2img,
                             dst, n, per_o / 8);
        else
          hipLaunchKernelGGL(rn_mul_gate_kernel, dim3(stream_grid((size_t)n * per_o)), dim3(256), 0, st, Ro, G, row2img,
                             (const float*)nullptr, dst, n, per_o);
        LRP_HIP_CHECK(hipGetLastError());
        return LRP_OK;
      };
      // S3 = R_o * (fA Q3) in s3 (r1 / r5), unless the epilogue of the block walked before this one has written it already
      // (same operand format: have_s3 is only set then); then S2 and S1.  S1 of a projection block takes the other S3 buffer,
      // which S0 follows into
      float* S1 = b.u0 < 0 ? r3.as<float>() : s3_other;
      if (!have_s3) LRP_TRY(head(b.GA.as<float>(), s3));
      LRP_TRY(unit_backward(units[b.u3], n, row2img, s3, units[b.u2].gate.as<float>(), r2.as<float>(), st, sp, !sp));              // S2
      LRP_TRY(unit_backward(units[b.u2], n, row2img, r2.as<float>(), units[b.u1].gate.as<float>(), S1, st, sp, !sp));              // S1
      if (b.u0 < 0) {
        // identity block, 3 conv launches: S3 -> S2 -> S1 -> R_t = t*C1 + R_o*GS, the join and (when the next block
        // agrees on the operand format) the next block's S3 = R_t * GA_next written by unit 1's epilogue
        BlockTail tl;
        tl.join = Ro; tl.join_gate = b.GS.as<float>();
        have_s3 = false;
        if (bi > 0 && block_split(blocks[bi - 1]) == sp) {
          tl.gate2 = blocks[bi - 1].GA.as<float>(); tl.out2 = s3_other;
          have_s3 = true;
        }
        LRP_TRY(unit_backward(units[b.u1], n, row2img, S1, b.t_in.as<float>(), cur, st, sp, true, &tl));
        std::swap(s3, s3_other);
        Ro = cur;
        std::swap(cur, other);
        continue;
      }
      // projection block (first of a stack)
      const float* taux = b.stride == 2 ? b.t_sub.as<float>() : b.t_in.as<float>();
      LRP_TRY(unit_backward(units[b.u1], n, row2img, S1, taux, r2.as<float>(), st, sp, true));                                    // t*C1 (coarse)
      LRP_TRY(head(b.GS.as<float>(), S1));                                                                                         // S0
      LRP_TRY(unit_backward(units[b.u0], n, row2img, S1, taux, r3.as<float>(), st, sp, true));                                    // t*C0
      // join: R_t = t*C1 + t*C0 (scattered to the even positions behind a stride-2 block) and — one pass — the head of the
      // block walked next, S3' = R_t * GA' (an identity block: the last of the stack below)
      have_s3 = false;
      const bool fuse_next = sp && bi > 0 && blocks[bi - 1].u0 < 0 && block_split(blocks[bi - 1]) && !(b.cin & 7);
      if (sp && !(b.cin & 7)) {
        const size_t tot8 = (size_t)n * b.Hin * b.Win * b.cin / 8;
        const float* g2 = fuse_next ? blocks[bi - 1].GA.as<float>() : (const float*)nullptr;
        float* o2 = fuse_next ? s3 : (float*)nullptr;    // (S3 of this block has been consumed)
        if (b.stride == 2)
          hipLaunchKernelGGL(rn_join_split_kernel<true>, dim3(stream_grid(tot8)), dim3(256), 0, st, r2.as<float>(), r3.as<float>(), cur,
                             g2, row2img, o2, n, b.Hin, b.Win, b.cin);
        else
          hipLaunchKernelGGL(rn_join_split_kernel<false>, dim3(stream_grid(tot8)), dim3(256), 0, st, r2.as<float>(), r3.as<float>(), cur,
                             g2, row2img, o2, n, b.Hin, b.Win, b.cin);
        have_s3 = fuse_next;
      } else if (b.stride == 2) {
        const size_t tot = (size_t)n * b.Hin * b.Win * b.cin;
        hipLaunchKernelGGL(rn_scatter2_kernel, dim3(stream_grid(tot)), dim3(256), 0, st, r2.as<float>(), r3.as<float>(), cur, n,
                           b.Hin, b.Win, b.cin);
      } else {
        const size_t per_c = (size_t)b.H * b.W * b.cin;
        hipLaunchKernelGGL(rn_add_kernel, dim3(stream_grid((size_t)n * per_c)), dim3(256), 0, st, r2.as<float>(), r3.as<float>(), cur,
                           (size_t)n * per_c);
      }
      LRP_HIP_CHECK(hipGetLastError());
      Ro = cur;
      std::swap(cur, other);
    }
    return stem_end(Ro, n, row2img, R_img_dev, st, false);
  }

  // ---- the stem conv's reverse, every walk's ----
  // r1 holds the operand S [n][Hout][Wout][K]: K = stem_c, or 2 stem_c where it carries two chains.  T = S . W over the 49 taps x 6
  // columns (w: w_b / w_bs, w_ab / w_abs, w_r / w_rs, w_g; rp: PREC_FP32, or PREC_BF16X3 for an operand and a matrix in split8 form), then
  // the 7x7 / stride-2 shift-and-add into the image.  (The kernels lie in the code object in the order the callers name them.)
  // The image end is the caller's: the instantiations of one MODE (resnet_kernels.h: 0 = LRP, x+ . T+ + x- . T-;  1 = T+, a
  // gradient, flat, w-square;  2 = x . T+;  3 = (x - low) . T+ + (x - high) . T-) — the stencil and the one-launch form for this operand (SPLIT = split8; nullptr: there is none)
  struct StemEnd {
    void (*fused)(const float*, const float*, const float*, const int*, float*, int, int, int, int, float, float);
    void (*stencil)(const float*, const float*, const int*, float*, int, int, int, float, float);
  };
  // the tap GEMM alone (explain_ab's dry run asks conv_plan about it)
  ConvArgs stem_tap_args(const float* w, int K, int n) const {
    const RnUnit& s = units[0];
    ConvArgs ca{};
    ca.in = r1.as<float>(); ca.NB = n * s.Hout * s.Wout; ca.H = 1; ca.W = 1; ca.Cin = K; ca.CinP = conv_cinp(K);
    ca.taps = 1; ca.wpk = w; ca.N = RN_STEM_TCOLS; ca.out = r2.as<float>();
    return ca;
  }
  // the dynamic-LDS attribute of an rn_stem_reverse_kernel instantiation, set before its first launch
  int stem_lds_attr(const void* kernel) {
    for (const void*& done : stem_attr_set) {
      if (done == kernel) return LRP_OK;
      if (done) continue;
      LRP_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RN_STEM_LDS));
      done = kernel;
      return LRP_OK;
    }
    return fail(LRP_ERR_STATE, "stem_lds_attr: more instantiations of rn_stem_reverse_kernel than slots");
  }
  // low, high: the BoundedRule's scalars (MODE 3 alone reads them)
  int stem_reverse(const float* w, int rp, int K, const StemEnd& end, int n, const int* row2img, float* R_img_dev, hipStream_t st,
                   float low = 0.f, float high = 0.f) {
    const RnUnit& s = units[0];
    // T = S . W and the shift-and-add in ONE launch, T never leaves LDS (resnet_kernels.h rn_stem_reverse_kernel): its K is fixed
    // at the 64 channels of one chain, so a two-chain operand (K = 2 stem_c) never takes it.  LRP_IMG_FUSED=0, and every other
    // stem: the two-kernel form below
    if (sw().img_fused != 0 && end.fused && w && K == s.cout && s.cout == 64 && conv_npad(RN_STEM_TCOLS) >= 5 * 60 + 4 &&
        conv_cinp(s.cout) == 64) {
      LRP_TRY(stem_lds_attr(reinterpret_cast<const void*>(end.fused)));
      const int txs = (s.Wout + RN_ST - 1) / RN_ST, tys = (s.Hout + RN_ST - 1) / RN_ST;
      hipLaunchKernelGGL(end.fused, dim3((unsigned)(n * txs * tys)), dim3(512), RN_STEM_LDS, st, r1.as<float>(), w, images.as<float>(),
                         row2img, R_img_dev, s.Hout, s.Wout, txs, tys, low, high);
      LRP_HIP_CHECK(hipGetLastError());
      return LRP_OK;
    }
    LRP_HIP_CHECK(conv_launch(EPI_STORE, stem_tap_args(w, K, n), st, rp));
    hipLaunchKernelGGL(end.stencil, dim3(stream_grid((size_t)n * img_h * img_w)), dim3(256), 0, st, r2.as<float>(), images.as<float>(),
                       row2img, R_img_dev, n, img_h, img_w, low, high);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  }

  // ---- the two-chain walk of the alpha-beta rule with beta > 0 (set_rule) ----
  // explain()'s walk with [S_a | S_i] tensors.  Per block: head S3 = R_o [GA | GA_i]; units 3 and 2 as dual-gate launches (one
  // accumulator c = convT(S_a, alpha w+) + convT(S_i, -beta w-), two gates, two outputs side by side); unit 1 and the projection
  // as ordinary one-gate launches over Cin = 2 cout whose output t * c is a relevance again.  The identity tail keeps the fused
  // join (R_o * GS: the shortcut has no conv, both chains share it); the next block's head is a pass of its own (two gates), or
  // rides on the projection join (rn_join2_kernel).  The stem: two-gate pool routing, the tap GEMM over K = 2 stem_c, the stencil.
  // dry: nothing is launched — conv_plan is asked about every conv launch of the walk, LRP_ERR_UNSUPPORTED for what it refuses.
  int explain_ab(int n, const int* row2img, const float* R_feat_dev, float* R_img_dev, hipStream_t st, bool dry) {
    const bool sp = prec == PREC_BF16X3;                 // (set_rule: every width is a multiple of 8)
    const int rp = sp ? PREC_BF16X3 : PREC_FP32;
    // one transposed conv through unit u over both chains; aux_b != nullptr: dual gate, the output carries two chains
    auto conv = [&](const RnUnit& u, const float* S, const float* aux, const float* aux_b, float* out, const BlockTail* tail) -> int {
      ConvArgs ca = bwd_args(u, n, row2img, S, out, 2);
      if (tail) { ca.join = tail->join; ca.join_gate = tail->join_gate; }
      ca.wpk = sp ? u.w_abs.as<float>() : u.w_ab.as<float>(); ca.aux = aux;
      if (aux_b) { ca.aux_b = aux_b; ca.out_b = out + u.cin; ca.ostride = 2 * u.cin; }
      else ca.out_plain = 1;                             // a relevance: feeds the join
      if (dry) {
        if (!conv_plan(conv_ask(EPI_MUL, rp, 7, false, ca)).ok)
          return fail(LRP_ERR_UNSUPPORTED, "alpha-beta walk: no conv kernel for '%s' (N=%d, Cin=%d, %s)", u.name.c_str(), ca.N, ca.Cin,
                      aux_b ? "dual gate" : "one gate");
        return LRP_OK;
      }
      prof.begin(st);
      LRP_HIP_CHECK(conv_launch(EPI_MUL, ca, st, rp));
      prof.end(st, 2 * bwd_flop(u, n));                  // (both chains)
      return LRP_OK;
    };
    auto head = [&](const RnBlock& bb, const float* Ro, const float* Ga, const float* Gi, float* dst) -> int {
      if (dry) return LRP_OK;
      const size_t per_o = (size_t)bb.H * bb.W * 4 * bb.f;
      if (sp)
        hipLaunchKernelGGL(rn_mul_gate2_kernel<true>, dim3(stream_grid((size_t)n * per_o / 8)), dim3(256), 0, st, Ro, Ga, Gi, row2img, dst, n,
                           per_o, 4 * bb.f);
      else
        hipLaunchKernelGGL(rn_mul_gate2_kernel<false>, dim3(stream_grid((size_t)n * per_o / 4)), dim3(256), 0, st, Ro, Ga, Gi, row2img, dst, n,
                           per_o, 4 * bb.f);
      LRP_HIP_CHECK(hipGetLastError());
      return LRP_OK;
    };
    const float* Ro = R_feat_dev;
    float *cur = r0.as<float>(), *other = r4.as<float>();
    float *s3 = r1.as<float>(), *s3_other = r5.as<float>();
    bool have_s3 = false;
    for (int bi = (int)blocks.size() - 1; bi >= 0; --bi) {
      const RnBlock& b = blocks[bi];
      const RnUnit &u1 = units[b.u1], &u2 = units[b.u2], &u3 = units[b.u3];
      if (!have_s3) LRP_TRY(head(b, Ro, b.GA.as<float>(), b.GA_i.as<float>(), s3));
      have_s3 = false;
      LRP_TRY(conv(u3, s3, u2.gate.as<float>(), u2.gate_i.as<float>(), r2.as<float>(), nullptr));                       // S2
      if (b.u0 < 0) {
        LRP_TRY(conv(u2, r2.as<float>(), u1.gate.as<float>(), u1.gate_i.as<float>(), r3.as<float>(), nullptr));         // S1
        BlockTail tl;
        tl.join = Ro; tl.join_gate = b.GS.as<float>();
        LRP_TRY(conv(u1, r3.as<float>(), b.t_in.as<float>(), nullptr, cur, &tl));                                       // R_t = t*C1 + R_o*GS
      } else {
        const RnUnit& u0 = units[b.u0];
        LRP_TRY(conv(u2, r2.as<float>(), u1.gate.as<float>(), u1.gate_i.as<float>(), s3_other, nullptr));               // S1
        const float* taux = b.stride == 2 ? b.t_sub.as<float>() : b.t_in.as<float>();
        LRP_TRY(conv(u1, s3_other, taux, nullptr, r2.as<float>(), nullptr));                                            // t*C1 (coarse)
        LRP_TRY(head(b, Ro, b.GS.as<float>(), b.GS_i.as<float>(), s3_other));                                           // S0
        LRP_TRY(conv(u0, s3_other, taux, nullptr, r3.as<float>(), nullptr));                                            // t*C0
        // join (scattered to the even positions behind a stride-2 block) and, in the same pass, the head of the block walked next
        const bool fuse_next = bi > 0;
        if (!dry) {
          const float* ga = fuse_next ? blocks[bi - 1].GA.as<float>() : (const float*)nullptr;
          const float* gi = fuse_next ? blocks[bi - 1].GA_i.as<float>() : (const float*)nullptr;
          float* o2 = fuse_next ? s3 : (float*)nullptr;
          const size_t tot = (size_t)n * b.Hin * b.Win * b.cin / (sp ? 8 : 4);
          const dim3 g(stream_grid(tot));
          const float *pa = r2.as<float>(), *pb = r3.as<float>();
          if (b.stride == 2 && sp)
            hipLaunchKernelGGL((rn_join2_kernel<true, true>), g, dim3(256), 0, st, pa, pb, cur, ga, gi, row2img, o2, n, b.Hin, b.Win, b.cin);
          else if (b.stride == 2)
            hipLaunchKernelGGL((rn_join2_kernel<true, false>), g, dim3(256), 0, st, pa, pb, cur, ga, gi, row2img, o2, n, b.Hin, b.Win, b.cin);
          else if (sp)
            hipLaunchKernelGGL((rn_join2_kernel<false, true>), g, dim3(256), 0, st, pa, pb, cur, ga, gi, row2img, o2, n, b.Hin, b.Win, b.cin);
          else
            hipLaunchKernelGGL((rn_join2_kernel<false, false>), g, dim3(256), 0, st, pa, pb, cur, ga, gi, row2img, o2, n, b.Hin, b.Win, b.cin);
          LRP_HIP_CHECK(hipGetLastError());
        }
        have_s3 = fuse_next;                              // (written into s3: S3 of this block has been consumed)
      }
      Ro = cur;
      std::swap(cur, other);
    }
    return stem_end(Ro, n, row2img, R_img_dev, st, dry);
  }

  // ---- the stem end of both LRP walks, chosen by the stem record alone: what arrives at the pool's output is a plain relevance
  // whatever the rule above it ----
  //   two chains (alpha-beta, beta > 0): two-gate pool routing -> T = [S_a | S_i] . [alpha (w+ | w-) ; -beta (w- | w+)] (K = 2 stem_c,
  //                N = 294) -> the 7x7/2 stencil with the x+ / x- selection
  //   one chain:   pool routing * q_stem -> T = S . W (K = stem_c) -> the image end of the record's MODE, in one launch where
  //                stem_reverse takes it.  W: w_b (alpha-beta, bounded) or w_r (epsilon, flat, w-square)
  // the tap GEMM runs as bf16x3 like the other convs of the walk: the pool routing writes its operand in split8 form (fp32 mode, and
  // a stem width that is no multiple of 8: plain fp32 on the fp32 MFMA).  dry: conv_plan is asked about the tap GEMM, nothing runs.
  int stem_end(const float* Ro, int n, const int* row2img, float* R_img_dev, hipStream_t st, bool dry) {
    const RnUnit& s = units[0];
    const Rule& r = rule_stem;
    const bool two = r.chains() == 2, own = !two && !r.on_default_matrix();
    const bool sp = prec == PREC_BF16X3 && !(s.cout & 7) && (two ? s.w_abs.p : own ? s.w_rs.p : s.w_bs.p) != nullptr;
    const int rp = sp ? PREC_BF16X3 : PREC_FP32, K = two ? 2 * s.cout : s.cout;
    const DevBuf& wm = two ? (sp ? s.w_abs : s.w_ab) : own ? (sp ? s.w_rs : s.w_r) : (sp ? s.w_bs : s.w_b);
    if (dry) {
      if (!conv_plan(conv_ask(EPI_STORE, rp, 7, false, stem_tap_args(wm.as<float>(), K, n))).ok)
        return fail(LRP_ERR_UNSUPPORTED, "LRP walk: no conv kernel for the stem's tap GEMM (K=%d)", K);
      return LRP_OK;
    }
    const size_t tot = (size_t)n * s.Hout * s.Wout * s.cout;
    const unsigned char* win = pool_win.as<unsigned char>();
    const float *qa = q_stem.as<float>(), *qi = q_stem_i.as<float>();
    float* S = r1.as<float>();
    if (two && sp)
      hipLaunchKernelGGL(rn_pool3_route2_kernel<true>, dim3(stream_grid(tot / 8)), dim3(256), 0, st, Ro, win, qa, qi, row2img, S, n, s.Hout,
                         s.Wout, s.cout);
    else if (two)
      hipLaunchKernelGGL(rn_pool3_route2_kernel<false>, dim3(stream_grid(tot / 4)), dim3(256), 0, st, Ro, win, qa, qi, row2img, S, n, s.Hout,
                         s.Wout, s.cout);
    else if (sp)
      hipLaunchKernelGGL(rn_pool3_route_kernel<true>, dim3(stream_grid(tot / 8)), dim3(256), 0, st, Ro, win, qa, row2img, S, n, s.Hout, s.Wout,
                         s.cout);
    else
      hipLaunchKernelGGL(rn_pool3_route_kernel<false>, dim3(stream_grid(tot / 4)), dim3(256), 0, st, Ro, win, qa, row2img, S, n, s.Hout, s.Wout,
                         s.cout);
    LRP_HIP_CHECK(hipGetLastError());
    StemEnd end{nullptr, &rn_stem_stencil_kernel<0>};
    switch (two ? LRP_RULE_ALPHA_BETA : r.kind) {
      case LRP_RULE_EPSILON: end = {sp ? &rn_stem_reverse_kernel<true, 2> : &rn_stem_reverse_kernel<false, 2>, &rn_stem_stencil_kernel<2>}; break;
      case LRP_RULE_FLAT:
      case LRP_RULE_WSQUARE: end = {sp ? &rn_stem_reverse_kernel<true, 1> : &rn_stem_reverse_kernel<false, 1>, &rn_stem_stencil_kernel<1>}; break;
      case LRP_RULE_BOUNDED: end = {sp ? &rn_stem_reverse_kernel<true, 3> : &rn_stem_reverse_kernel<false, 3>, &rn_stem_stencil_kernel<3>}; break;
      default: if (!two) end.fused = sp ? &rn_stem_reverse_kernel<true> : &rn_stem_reverse_kernel<false>;
    }
    return stem_reverse(wm.as<float>(), rp, K, end, n, row2img, R_img_dev, st, r.low, r.high);
  }

  // ---- gradient walks (lrp_cnn_walk: LRP_WALK_GRADIENT / _INPUT_X_GRADIENT / _GUIDED_BACKPROP) -------------------------------
  // w_g of every unit whose weights changed since its last packing, from the device-resident forward matrix w_a and the BN
  // vectors (no host copy of the weights is kept; LRP-only users never allocate or pack these)
  int ensure_grad_weights(hipStream_t st) {
    for (RnUnit& u : units) {
      if (u.grad_ok) continue;
      if (u.k == 7) {
        const int Npb = conv_npad(RN_STEM_TCOLS), Kb = conv_cinp(u.cout);
        const size_t nb = (size_t)Npb * Kb;
        LRP_TRY(reserve(u.w_g, nb));
        hipLaunchKernelGGL(rn_pack_stem_grad_kernel, dim3(stream_grid(nb)), dim3(256), 0, st, u.w_a.as<float>(), u.gamma.as<float>(),
                           u.var.as<float>(), RN_BN_EPS, u.w_g.as<float>(), u.cout, Npb, Kb);
      } else {
        const int taps = u.k * u.k, CPi = conv_cinp(u.cin), CPo = conv_cinp(u.cout), rows = conv_npad(u.cin);
        const size_t nb = (size_t)rows * taps * CPo;
        LRP_TRY(reserve(u.w_g, nb));
        hipLaunchKernelGGL(rn_pack_grad_kernel, dim3(stream_grid(nb)), dim3(256), 0, st, u.w_a.as<float>(), u.gamma.as<float>(),
                           u.var.as<float>(), RN_BN_EPS, u.w_g.as<float>(), taps, u.cin, u.cout, CPi, CPo, rows);
      }
      LRP_HIP_CHECK(hipGetLastError());
      u.grad_ok = true;
    }
    return LRP_OK;
  }
  // one unit's gradient step: out = convT(S, W s) on the unit's output grid, then the ReLU in front of it — clamp: at 0 first
  // (GUIDED, Deconvnet); mask != nullptr: its forward decision — and (tail != nullptr, with a mask) the residual join
  // out = rho(acc + tail) [mask], all in the conv's epilogue
  int grad_backward(const RnUnit& u, int n, const int* row2img, const float* S, const unsigned char* mask, float* out, bool clamp,
                    hipStream_t st, const float* tail = nullptr) {
    ConvArgs ca = bwd_args(u, n, row2img, S, out);
    ca.wpk = u.w_g.as<float>(); ca.out_plain = 1; ca.relu_out = clamp ? 1 : 0;
    if (!mask) {
      ca.gate_none = 1;
      LRP_HIP_CHECK(conv_launch(EPI_MUL, ca, st, PREC_FP32));
      return LRP_OK;
    }
    ca.aux = reinterpret_cast<const float*>(mask);       // (byte masks: conv_igemm_kernel GMASK)
    if (tail) { ca.join = tail; ca.join_gate = reinterpret_cast<const float*>(mask); }
    LRP_HIP_CHECK(conv_launch_grad_mask(ca, st));
    return LRP_OK;
  }
  // The walk (oracle: tests/resnet_grad_ref.py).  One tensor per block boundary: G = the gradient at the block's pre-ReLU sum,
  // which is both the head of the block's chain and its shortcut's term of the join below.
  //   identity block:   G' = [t_in > 0] rho( convT1([a1 > 0] rho(convT2([a2 > 0] rho(convT3(G))))) + G )
  //   projection block: the same main chain and convT0(G) on the coarse grid, summed (scattered to the even positions behind a
  //                     stride 2) BEFORE the block input's ReLU; the first block's input is the stem pool's output: no ReLU
  //   stem:             pool routing summed over the overlapping windows, rho, [a0 > 0], convT of the 7x7/2 conv, crop
  // rho = relu for GUIDED_BACKPROP (every ReLU clamps what arrives first), identity otherwise.
  // LRP_WALK_DECONVNET (gradient_based.py:180-225) is the GUIDED walk with every mask replaced by ones: rho at each Activation,
  // the plain gradient through conv + BN, Add, pad and the stem pool.  It reads no ReLU decision — only pool_win, which every
  // forward writes, and the BN-scaled matrices — so it runs in every precision mode.
  // What the four walks disagree on, decided once at the top of explain_grad:
  struct GradMode {
    bool masks = true;     // the fp32 forward's ReLU decisions are read (off: Deconvnet)
    int clamp = 0;         // what a ReLU does to what arrives: 0 nothing but its mask, 1 GUIDED: clamp, then the mask,
                           // 2 Deconvnet: the clamp alone (rn_grad_join_kernel tells 1 from 2; everywhere else it is a flag)
    int img_mode = 1;      // the image end (rn_stem_reverse_kernel's MODE): 1 the gradient, 2 times the image
  };
  int explain_grad(int n, const int* row2img, const float* head, float* R_img_dev, hipStream_t st, int walk) {
    if (walk != LRP_WALK_GRADIENT && walk != LRP_WALK_INPUT_X_GRADIENT && walk != LRP_WALK_GUIDED_BACKPROP && walk != LRP_WALK_DECONVNET)
      return fail(LRP_ERR_INVALID, "unknown walk %d", walk);
    GradMode m;
    m.masks = walk != LRP_WALK_DECONVNET;
    m.clamp = walk == LRP_WALK_DECONVNET ? 2 : walk == LRP_WALK_GUIDED_BACKPROP ? 1 : 0;
    m.img_mode = walk == LRP_WALK_INPUT_X_GRADIENT ? 2 : 1;
    if (m.masks && prec != PREC_FP32)
      return fail(LRP_ERR_UNSUPPORTED, "gradient walks on a ResNet encoder run in LRP_PREC_FP32 only: set it with lrp_set_precision "
                                       "and call lrp_encode_images again");
    if (m.masks && !masks_ok)
      return fail(LRP_ERR_STATE, "lrp_encode_images must run in LRP_PREC_FP32 mode before a ResNet gradient walk");
    auto mask_of = [&](const DevBuf& d) { return m.masks ? d.as<unsigned char>() : (const unsigned char*)nullptr; };
    const bool clamp = m.clamp != 0;
    LRP_TRY(ensure_grad_weights(st));
    float* G = r0.as<float>();
    float* other = r4.as<float>();
    {
      const RnBlock& t = blocks.back();
      const size_t per = (size_t)t.H * t.W * 4 * t.f;
      hipLaunchKernelGGL(rn_grad_head_kernel, dim3(stream_grid((size_t)n * per / 4)), dim3(256), 0, st, head, mask_of(t.omask), row2img, G,
                         n, per, clamp ? 1 : 0);
      LRP_HIP_CHECK(hipGetLastError());
    }
    for (int bi = (int)blocks.size() - 1; bi >= 0; --bi) {
      const RnBlock& b = blocks[bi];
      const RnUnit &u1 = units[b.u1], &u2 = units[b.u2], &u3 = units[b.u3];
      LRP_TRY(grad_backward(u3, n, row2img, G, mask_of(u2.mask), r2.as<float>(), clamp, st));
      LRP_TRY(grad_backward(u2, n, row2img, r2.as<float>(), mask_of(u1.mask), r3.as<float>(), clamp, st));
      // the block input's ReLU (the first block's input is the stem pool's output: none there)
      const unsigned char* in_mask = bi > 0 ? mask_of(blocks[bi - 1].omask) : (const unsigned char*)nullptr;
      if (m.masks && b.u0 < 0) {
        // identity block (never the first) with masks: the join and the block input's ReLU ride in unit 1's epilogue
        LRP_TRY(grad_backward(u1, n, row2img, r3.as<float>(), in_mask, other, clamp, st, G));
      } else {
        LRP_TRY(grad_backward(u1, n, row2img, r3.as<float>(), nullptr, r1.as<float>(), false, st));
        const float* sc = G;                             // the shortcut's term: G itself, or convT0(G) on the coarse grid
        if (b.u0 >= 0) {
          LRP_TRY(grad_backward(units[b.u0], n, row2img, G, nullptr, r5.as<float>(), false, st));
          sc = r5.as<float>();
        }
        // the join, then the block input's ReLU
        const size_t tot = (size_t)n * b.Hin * b.Win * b.cin / 4;
        const int jclamp = m.masks || bi > 0 ? m.clamp : 0;
        if (b.u0 >= 0 && b.stride == 2)
          hipLaunchKernelGGL(rn_grad_join_kernel<true>, dim3(stream_grid(tot)), dim3(256), 0, st, r1.as<float>(), sc, in_mask, row2img, other,
                             n, b.Hin, b.Win, b.cin, jclamp);
        else
          hipLaunchKernelGGL(rn_grad_join_kernel<false>, dim3(stream_grid(tot)), dim3(256), 0, st, r1.as<float>(), sc, in_mask, row2img, other,
                             n, b.Hin, b.Win, b.cin, jclamp);
        LRP_HIP_CHECK(hipGetLastError());
      }
      std::swap(G, other);
    }
    // stem: G is the gradient at the pool's output
    const RnUnit& s = units[0];
    const size_t tot = (size_t)n * s.Hout * s.Wout * s.cout / 4;
    hipLaunchKernelGGL(rn_grad_pool_route_kernel, dim3(stream_grid(tot)), dim3(256), 0, st, G, pool_win.as<unsigned char>(),
                       m.masks ? a0.as<float>() : (const float*)nullptr, row2img, r1.as<float>(), n, s.Hout, s.Wout, s.cout, clamp ? 1 : 0);
    LRP_HIP_CHECK(hipGetLastError());
    const StemEnd end{m.img_mode == 1 ? &rn_stem_reverse_kernel<false, 1> : &rn_stem_reverse_kernel<false, 2>,
                      m.img_mode == 2 ? &rn_stem_stencil_kernel<2> : &rn_stem_stencil_kernel<1>};
    return stem_reverse(s.w_g.as<float>(), PREC_FP32, s.cout, end, n, row2img, R_img_dev, st);
  }
};

}  // namespace lrp
