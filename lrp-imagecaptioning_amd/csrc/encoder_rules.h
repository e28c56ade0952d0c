// encoder_rules.h — the rule table of the VGG walk (lrp_set_cnn_rule, lrp_set_cnn_rules): one rule per conv.
// State: RuleTableState (encoder_state.h), Encoder::rules.  set_table / clear_table, the table's operand copies
// (pack_table_layer), its gates behind the forward (table_pass, called by encode) and its walk (rule_head, explain_table).
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
// Included by encoder.h behind struct Encoder.
#pragma once
namespace lrp {
inline void Encoder::clear_table() {
  if (!table_on()) return;
  rules.table.clear();                                 // (the buffers stay, idle; the other users' requests for the activations stand)
  keep_acts = acts_wanted();
  encoded = 0;                                         // the caches belong to the old rule
}
// `t` is validated (engine.hip) and not empty
inline int Encoder::set_table(const std::vector<ConvRule>& t, int64_t* total) {
  // a buffer appears, or grows, with the first table that needs it at that size: everything is sized by THIS table's chain counts
  auto mk = [&](DevBuf& d, size_t floats) { return grow(d, floats * sizeof(float), total, 1); };
  const size_t B = (size_t)max_images, NT = (size_t)max_tokens, nl = layers.size();
  for (size_t i = 0; i < nl; ++i) {
    ConvLayer& L = layers[i];
    RuleTableState::Layer& tl = rules.layer[i];
    const ConvRule& r = t[i];
    const bool top = i + 1 == nl;
    const int k = r.chains();
    if (!top && r.own_gate()) LRP_TRY(mk(tl.Gt, B * L.act_elems()));
    if (!top && k == 2) LRP_TRY(mk(tl.Gn, B * L.act_elems()));
    const size_t nf = i == 0 ? (size_t)conv_npad(L.cout) * 64 : (size_t)conv_npad(L.cout) * 9 * conv_cinp(L.cin);
    const size_t nb = i == 0 ? (size_t)conv_npad(IMG_T_COLS) * conv_cinp(k * L.cout) : (size_t)conv_npad(L.cin) * 9 * conv_cinp(k * L.cout);
    if (r.fwd_a()) { LRP_TRY(mk(tl.w_fwd_t, nf)); if (i) LRP_TRY(mk(tl.w_fwd_ts, nf)); }
    if (k == 2) { LRP_TRY(mk(tl.w_fwd_n, nf)); if (i) LRP_TRY(mk(tl.w_fwd_ns, nf)); }
    if (!r.on_default_matrix()) { LRP_TRY(mk(tl.w_bwd_t, nb)); LRP_TRY(mk(tl.w_bwd_t_s, nb)); }
    tl.packed = false;
  }
  if (t.back().own_gate()) LRP_TRY(mk(rules.zt_top, B * layers.back().act_elems()));
  if (t.back().chains() == 2) LRP_TRY(mk(rules.zntop, B * layers.back().act_elems()));
  if (t[0].kind == LRP_RULE_WSQUARE) LRP_TRY(mk(rules.wsq_zc, (size_t)16 * layers[0].cout));
  if (t[0].kind == LRP_RULE_BOUNDED) LRP_TRY(mk(rules.a1b, B * img_h * img_w * 64));
  if (RuleTableState::chains_of(t) == 2) {             // (one chain everywhere: the default walk's ping-pong s0 / s1)
    const size_t tok = std::max(2 * max_act_elems(), (size_t)img_h * img_w * IMG_T_COLS);
    LRP_TRY(mk(rules.s0ab, NT * tok)); LRP_TRY(mk(rules.s1ab, NT * tok));
  }
  LRP_TRY(alloc_keep_acts(total));
  keep_acts = true;
  rules.table = t;
  encoded = 0;
  return LRP_OK;
}
// the table's operand copies of layer li from w_dev (HWIO, device)
inline int Encoder::pack_table_layer(int li, const float* w_dev, hipStream_t st) {
  ConvLayer& L = layers[li];
  RuleTableState::Layer& tl = rules.layer[li];
  const ConvRule& r = rules.table[li];
  const int k = r.chains();
  auto split = [&](const float* src, float* dst, size_t n) {
    hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(n / 8)), dim3(256), 0, st, src, dst, n / 8);
  };
  const bool fwd_a = r.fwd_a();
  const bool own_bwd = !r.on_default_matrix();
  if (own_bwd) {                                       // the last table's layout may have been another: cleared in stream order
    LRP_HIP_CHECK(hipMemsetAsync(tl.w_bwd_t.p, 0, tl.w_bwd_t.bytes, st));
    LRP_HIP_CHECK(hipMemsetAsync(tl.w_bwd_t_s.p, 0, tl.w_bwd_t_s.bytes, st));
  }
  if (li == 0) {
    const int Kb = conv_cinp(k * L.cout);
    if (!own_bwd) { tl.packed = true; return LRP_OK; }   // (alpha-beta (1, 0) with bias needs nothing of its own)
    hipLaunchKernelGGL(pack_image_layer_rule_dev_kernel, dim3((27 * L.cout + 255) / 256), dim3(256), 0, st, w_dev,
                       fwd_a ? tl.w_fwd_t.as<float>() : (float*)nullptr, k == 2 ? tl.w_fwd_n.as<float>() : (float*)nullptr, tl.w_bwd_t.as<float>(),
                       L.cout, Kb, r.kind, k, r.alpha, r.beta);
    split(tl.w_bwd_t.as<float>(), tl.w_bwd_t_s.as<float>(), (size_t)conv_npad(IMG_T_COLS) * Kb);
    if (r.kind == LRP_RULE_WSQUARE)
      hipLaunchKernelGGL(wsquare_class_kernel, dim3((16 * L.cout + 255) / 256), dim3(256), 0, st, w_dev, rules.wsq_zc.as<float>(), L.cout);
  } else {
    const int CPi = conv_cinp(L.cin), CPk = conv_cinp(k * L.cout);
    const size_t nf = (size_t)conv_npad(L.cout) * 9 * CPi, nb = (size_t)conv_npad(L.cin) * 9 * CPk;
    auto pack = [&](float* dst, int bwd, int chains, float p0, float q0, float p1, float q1) {
      const int rows = bwd ? L.cin : L.cout, CP = bwd ? CPk : CPi;
      hipLaunchKernelGGL(pack_conv_rule_dev_kernel, dim3(stream_grid((size_t)rows * 9 * CP)), dim3(256), 0, st, w_dev, dst, bwd, L.cin, L.cout, CP,
                         rows, chains, p0, q0, p1, q1);
    };
    if (fwd_a) { pack(tl.w_fwd_t.as<float>(), 0, 1, 1.f, 0.f, 0.f, 0.f); split(tl.w_fwd_t.as<float>(), tl.w_fwd_ts.as<float>(), nf); }
    if (k == 2) { pack(tl.w_fwd_n.as<float>(), 0, 1, 0.f, 1.f, 0.f, 0.f); split(tl.w_fwd_n.as<float>(), tl.w_fwd_ns.as<float>(), nf); }
    if (own_bwd) {
      if (r.kind == LRP_RULE_EPSILON) pack(tl.w_bwd_t.as<float>(), 1, 1, 1.f, 1.f, 0.f, 0.f);
      else if (k == 2) pack(tl.w_bwd_t.as<float>(), 1, 2, r.alpha, 0.f, 0.f, -r.beta);
      else pack(tl.w_bwd_t.as<float>(), 1, 1, 1.f, 0.f, 0.f, 0.f);          // (alpha-beta (1, 0) without the bias: w+)
      split(tl.w_bwd_t.as<float>(), tl.w_bwd_t_s.as<float>(), nb);
    }
  }
  LRP_HIP_CHECK(hipGetLastError());
  tl.packed = true;
  return LRP_OK;
}
// Behind the forward (keep_acts: every conv's input is still there): per layer the denominators its rule needs beyond the forward's
// Z+ — over the kept layer inputs, exact fp32 or three-term split-bf16 like the Z+ convs of the mixed modes with the handle
// (epsilon tables: fp32; the image layer's GEMM stays fp32 as in every forward) — and the gates from them.  A pooled layer's
// gates take the arg-max mask from G+; the top layer has no gate, its denominators stay next to ztop.
inline int Encoder::table_pass(int B, hipStream_t st) {
  LRP_TRY(wait_gates(st, true));
  const bool split = table_split();
  for (size_t li = 0; li < layers.size(); ++li) {
    ConvLayer& L = layers[li];
    RuleTableState::Layer& tl = rules.layer[li];
    const ConvRule& r = rules.table[li];
    if (!tl.packed) {
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
                           rules.a1b.as<float>(), B, img_h, img_w, r.low, r.high);
        LRP_HIP_CHECK(hipGetLastError());
        cz = ConvArgs{};
        cz.in = rules.a1b.as<float>(); cz.NB = B * L.H * L.W; cz.H = 1; cz.W = 1; cz.Cin = 64; cz.CinP = 64; cz.taps = 1;
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
                         rules.wsq_zc.as<float>(), out, B, L.H, L.W, L.cout, zmode, r.eps);
      LRP_HIP_CHECK(hipGetLastError());
      return LRP_OK;
    };
    float* zbuf = bufZ.as<float>();
    if (r.own_gate()) {                                // the activator chain
      float* zdst = top ? rules.zt_top.as<float>() : zbuf;
      float* gdst = fuse ? tl.Gt.as<float>() : zdst;    // (a v / safe(z) gate)
      switch (r.kind) {
        case LRP_RULE_ALPHA_BETA:                      // without the bias: conv(x+, w+) + conv(x-, w-)
          LRP_TRY(den_conv(tl.w_fwd_t.as<float>(), tl.w_fwd_ts.as<float>(), false, false, gdst, fuse));
          if (!top && !fuse) LRP_TRY(gate(zbuf, 0, tl.Gt.as<float>()));
          break;
        case LRP_RULE_BOUNDED:
          LRP_TRY(den_conv(tl.w_fwd_t.as<float>(), nullptr, false, true, gdst, fuse));
          if (!top && !fuse) LRP_TRY(gate(zbuf, 0, tl.Gt.as<float>()));
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
              LRP_TRY(gate(zbuf, 1, tl.Gt.as<float>()));
            }
          } else {
            LRP_TRY(gate(nullptr, 2, tl.Gt.as<float>()));
          }
          break;
        case LRP_RULE_FLAT: LRP_TRY(gate(nullptr, 3, tl.Gt.as<float>())); break;
        case LRP_RULE_WSQUARE: LRP_TRY(gate(nullptr, 4, tl.Gt.as<float>())); break;
      }
    }
    if (r.chains() == 2) {                             // the inhibitor chain: conv(x+, w-) + conv(x-, w+), with the bias or without
      LRP_TRY(den_conv(tl.w_fwd_n.as<float>(), tl.w_fwd_ns.as<float>(), r.bias != 0, false,
                       top ? rules.zntop.as<float>() : fuse ? tl.Gn.as<float>() : zbuf, fuse));
      if (!top && L.pool_after) {
        const size_t n4 = (size_t)B * L.act_elems() / 4;
        hipLaunchKernelGGL(pool_gate_inh_kernel, dim3(stream_grid(n4)), dim3(256), 0, st, L.G.as<f32x4>(), L.P.as<float>(),
                           reinterpret_cast<const f32x4*>(zbuf), tl.Gn.as<f32x4>(), B, L.H, L.W, L.cout);
        LRP_HIP_CHECK(hipGetLastError());
      }
    }
  }
  return LRP_OK;
}
// head of a rule's walk (KG:898-900 per chain): S_top = R / safe(den_top[img]) in the form the top layer's launch reads
inline int Encoder::rule_head(const ConvRule& r, bool split, int n, const int* row2img_dev, const float* R_feat_dev, float* S, hipStream_t st) {
  const ConvLayer& T = layers.back();
  const float* za = r.own_gate() ? rules.zt_top.as<float>() : ztop.as<float>();
  const size_t pixels = (size_t)n * T.H * T.W, per = T.act_elems();
  if (r.chains() == 2) {
    const size_t items = pixels * (T.cout / (split ? 8 : 4));
    if (split)
      hipLaunchKernelGGL(chain_join_kernel<true>, dim3(stream_grid(items)), dim3(256), 0, st, R_feat_dev, R_feat_dev, za, rules.zntop.as<float>(),
                         row2img_dev, S, pixels, T.H * T.W, T.cout);
    else
      hipLaunchKernelGGL(chain_join_kernel<false>, dim3(stream_grid(items)), dim3(256), 0, st, R_feat_dev, R_feat_dev, za, rules.zntop.as<float>(),
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
inline int Encoder::explain_table(int n, const int* row2img_dev, const float* R_feat_dev, float* R_img_dev, hipStream_t st) {
  if (walk_f16) return fail(LRP_ERR_UNSUPPORTED, "LRP_PREC_F16X2 has no rule-table walk (its per-token scaling is per chain)");
  if (!table_runs()) return fail(LRP_ERR_UNSUPPORTED, "epsilon rules run in LRP_PREC_FP32 only");
  const bool split = table_split();
  const int rp = split ? PREC_BF16X3 : PREC_FP32, nl = (int)layers.size();
  float *S, *Snext;
  chain_buffers(RuleTableState::chains_of(rules.table) == 2, S, Snext);
  // layer li reads its rule's chains against its rule's matrix — li >= 1: into the gate(s) of the rule below
  auto conv_args = [&](int li) {
    const ConvLayer& L = layers[li];
    ConvArgs ca = conv3x3_args(L, n, S, rules.table[li].chains() * L.cout);
    ca.wpk = rule_matrix(li, split); ca.row2img = row2img_dev;
    if (li == 0) return ca;
    ca.N = L.cin; ca.aux = table_gate(li - 1); ca.out = Snext;
    if (rules.table[li - 1].chains() == 2) { ca.aux_b = rules.layer[li - 1].Gn.as<float>(); ca.out_b = Snext + L.cin; ca.ostride = 2 * L.cin; }
    return ca;
  };
  LRP_TRY(plan_or_refuse(1, nl, n, rp, conv_args, [&](int li) {
    return fail(LRP_ERR_UNSUPPORTED, "conv %d: no launch reads %d chain(s) of %d channels into %d gate(s)", li, rules.table[li].chains(),
                layers[li].cout, rules.table[li - 1].chains());
  }));
  LRP_TRY(rule_head(rules.table.back(), split, n, row2img_dev, R_feat_dev, S, st));
  for (int li = nl - 1; li >= 1; --li) {
    if (layers[li - 1].pool_after) LRP_TRY(full_gate(li - 1, st));
    const ConvArgs ca = conv_args(li);
    LRP_TRY(timed_conv(mul_epi(li, ca), ca, st, rp, (double)rules.table[li].chains() * layer_flop(n, li)));
    std::swap(S, Snext);
  }
  const ConvRule& r0 = rules.table[0];
  return image_layer_step(conv_args(0), n, rp, (double)r0.chains() * layer_flop(n, 0), Snext, R_img_dev, r0.img_mode(), r0.low, r0.high, st);
}
}  // namespace lrp
