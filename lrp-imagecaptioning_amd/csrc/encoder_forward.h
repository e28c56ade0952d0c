// encoder_forward.h — the forward once per image: the four paths Encoder::encode() chooses from (fwd_mode.h) and the launch
// helpers they share.  forward_exact (LRP_PREC_FP32), forward_fast (LRP_PREC_BF16X3_FAST: activation chain on the caller's stream,
// denominators and gates on the side stream), forward_pairs_split and forward_pairs_emit (the fp16-pair dual forward, the default).
// Encoder::fwd_fast — the first layer whose ACTIVATION conv runs split-bf16 too.  A ~1e-5 relative error in a_l is harmless by
// itself, but upstream of a 2x2 max-pool it flips the arg-max of near-tied windows (~1e-5 of them), and a flipped window moves
// its whole relevance to a neighbour pixel: measured on VGG16, relative L1 of the heat-maps 5e-6 ... 3.6e-5 instead
// of 5.6e-6.  Default: none (splitting only the layers behind the last pool is flip-free but makes the features the
// decoder consumes 10x less exact, 7.4e-7 -> 7.8e-6, for 0.5 ms); lrp_set_precision(LRP_PREC_BF16X3_FAST): every layer
// but the image layer (-5 ms, heat-map parity <= 4e-5): forward_fast.
// The fp16-pair forwards — activation chain and denominators in ONE pass on the fp16 MFMA: operands as fp16 pairs hi + lo (22
// mantissa bits, x scaled by a power of two per layer and image), product hi*hi' + hi*lo' + lo*hi' in three MFMAs with blocked
// fp32 accumulation, weights (w | w+) stacked along N; with interleaved weight rows (Encoder::fwd_il) a_l and the gate
// G_l = a_l / safe(Z+_l) leave the conv's epilogue together where no pool follows (conv_args.h ConvArgs::dual_il) — no Z+ tensor,
// no gate pass.  LRP_FWD_IL=0: stacked rows.
// fwd_terms — the denominators Z+_l of the layers whose reverse launch is two-term (explain(): up to the last pool, >= 576
// products) are computed two-term as well, with the SAME rounded weights hi(w+) the walk multiplies with.
// [MI355X: parity at the bench configuration 5.5e-6 -> 4.4e-6, 6 seeds median 4.2e-6 -> 3.3e-6: gate and
// transposed conv now belong to one (slightly perturbed) network and the rounding largely cancels in R / Z+;
// two-term Z+ in EVERY layer: 1.0e-4, the top block again.]
// Included by encoder.h behind struct Encoder.
#pragma once
namespace lrp {
inline ConvArgs Encoder::fwd_conv_args(const ConvLayer& L, int B, const float* in) {
  ConvArgs ca = conv3x3_args(L, B, in, L.cin);
  ca.bias = L.bias.as<float>();
  return ca;
}
// the image layer as a GEMM over its im2col matrix a1 (one row per pixel, 64 columns: 27 x+ | 27 x- | padding)
inline int Encoder::im2col_gemm_args(int B, hipStream_t st, ConvArgs& ca) {
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
inline int Encoder::gate_pass(ConvLayer& L, int B, const float* a, const float* z, hipStream_t st) {
  const size_t n = (size_t)B * L.act_elems();
  hipLaunchKernelGGL(gate_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(a),
                     reinterpret_cast<const f32x4*>(z), L.G.as<f32x4>(), n / 4);
  return launched();
}
// arg-max gate of a pooled layer at full resolution; pooled != nullptr: pool(a_l) as well
inline int Encoder::pool_gate_pass(ConvLayer& L, int B, const float* a, const float* z, float* pooled, hipStream_t st) {
  const size_t n = (size_t)B * L.act_elems();
  hipLaunchKernelGGL(pool_gate_kernel, dim3(stream_grid(n / 16)), dim3(256), 0, st, a, z, pooled, L.G.as<float>(), B, L.H, L.W, L.cout);
  return launched();
}
inline int Encoder::maxpool_pass(ConvLayer& L, int B, const float* a, hipStream_t st) {
  const size_t n = (size_t)B * L.act_elems();
  hipLaunchKernelGGL(maxpool2_kernel, dim3(stream_grid(n / 16)), dim3(256), 0, st, a, L.P.as<float>(), B, L.H, L.W, L.cout);
  return launched();
}
inline int Encoder::split_copy(const float* src, size_t n8, hipStream_t st) {      // split8 (bf16 hi | lo) copy of a conv input into bufXs
  hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(n8)), dim3(256), 0, st, src, bufXs.as<float>(), n8);
  return launched();
}
// a_l where the gate pass of a layer finds it when the conv parked it in the gate's own storage
inline const float* Encoder::parked_act(const ConvLayer& L) const { return keep_acts ? L.Akeep.as<float>() : L.G.as<float>(); }
// where a layer's activation conv of the overlapped forwards writes a_l: the features, where the fine-tune step looks for
// it, or parked in the storage of its future gate
inline float* Encoder::act_out(ConvLayer& L, bool top) { return top ? feat.as<float>() : (keep_acts && !L.pool_after) ? L.Akeep.as<float>() : L.G.as<float>(); }
// One layer of the exact forward, and the image layer of every forward that does not emit: dual fp32 GEMM (a_l | Z+_l), gate
// or pool-gate pass, x / a ping-pong.  On return x holds the next conv's input.
inline int Encoder::dual_fp32_layer(size_t li, int B, hipStream_t st, float*& x, float*& a, float* z) {
  ConvLayer& L = layers[li];
  const bool top = li + 1 == layers.size();
  ConvArgs ca;
  if (li == 0) LRP_TRY(im2col_gemm_args(B, st, ca));
  else ca = fwd_conv_args(L, B, x);
  ca.wpk = L.w_fwd.as<float>(); ca.N = 2 * L.cout; ca.split = L.cout;
  ca.out = top ? feat.as<float>() : a; ca.out2 = top ? ztop.as<float>() : z;
  if (dl.capture && li > 0)                            // the reference's forward: its input of this layer ...
    LRP_HIP_CHECK(hipMemcpyAsync(dl.layer[li].Xr.p, x, (size_t)L.H * L.W * L.cin * sizeof(float), hipMemcpyDeviceToDevice, st));
  LRP_HIP_CHECK(conv_launch(EPI_FWD_DUAL, ca, st));
  if (dl.capture)                                      // ... and its activation, in front of the pool
    LRP_HIP_CHECK(hipMemcpyAsync(dl.layer[li].Yr.p, top ? feat.p : (void*)a, L.act_elems() * sizeof(float), hipMemcpyDeviceToDevice, st));
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
inline int Encoder::forward_exact(int B, hipStream_t st) {
  float *x = bufX.as<float>(), *a = bufA.as<float>();
  for (size_t li = 0; li < layers.size(); ++li) LRP_TRY(dual_fp32_layer(li, B, st, x, a, bufZ.as<float>()));
  return LRP_OK;
}
// LRP_PREC_BF16X3_FAST: the caller's stream runs the activation chain a_1..a_top alone, split-bf16 behind the image layer (its
// error passes through few further layers); the denominators and the gates follow on the side stream.
inline int Encoder::forward_fast(int B, hipStream_t st) {
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
// the dual conv a_l | Z+_l of layer li >= 1 over the pairs in `pin`; a_l goes to act_out, Z+_l to ztop / bufZ
inline ConvArgs Encoder::dual_pairs_args(size_t li, int B, const float* pin, const ScaleRecs& r, bool per_img) {
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
inline void Encoder::fuse_gate(ConvLayer& L, ConvArgs& cd, const float* x_in) {
  if (!keep_acts) cd.out = x_in == bufA.as<float>() ? bufX.as<float>() : bufA.as<float>();
  cd.out2 = L.G.as<float>(); cd.dual_gate = 1;
}
inline int Encoder::fwd_terms(size_t li, const ConvArgs& cd) const { return cd.dual_il && walk_f16 && two_term((int)li) ? 23 : 7; }
// behind the pool gate of layer li, fused into the conv or a pass of its own: what this encode left for the walks
inline int Encoder::after_pool_gate(size_t li, int B, hipStream_t st, bool full_written) {
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
inline int Encoder::forward_pairs_split(int B, hipStream_t st) {
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
inline int Encoder::forward_pairs_emit(int B, hipStream_t st) {
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
inline int Encoder::image_layer_emit(int B, hipStream_t st, const ScaleRecs& r, float* pairs_out) {
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
}  // namespace lrp
