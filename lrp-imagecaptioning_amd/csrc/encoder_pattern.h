// encoder_pattern.h — PatternNet / PatternAttribution for the VGG encoder (lrp_pattern_*, LRP_WALK_PATTERNNET /
// _PATTERN_ATTRIBUTION; pattern_kernels.h).  State: PatternState (encoder_state.h), Encoder::pat.
// The fit and the walk are independent: the walk takes whatever patterns the layers hold, fitted here or set by the caller.
// Everything is allocated by the first pattern call that needs it; a handle that never makes one allocates nothing.  While a fit
// is open (pat.type >= 0) the handle is one more user of keep_acts.
// The walk (explain_pattern; pattern_based.py:68-125): per conv + ReLU layer the ReLU's gradient, then the conv's gradient with the
// kernel replaced by A (PatternNet) or A * w (PatternAttribution); every reversed tensor is divided by its row's absolute maximum
// first (pat.project; the head, every conv's input, the result — behind a pool the routed tensor's maximum is already 1).
// Included by encoder.h behind struct Encoder.
#pragma once
namespace lrp {
inline int Encoder::pattern_mode_check() const {
  if (prec != PREC_FP32)
    return fail(LRP_ERR_UNSUPPORTED, "the pattern fit and walks run in LRP_PREC_FP32 only (a mask taken in another arithmetic is another mask): "
                                     "set it with lrp_set_precision and call lrp_encode_images again");
  return LRP_OK;
}
inline int Encoder::pattern_fit_begin(int type, int64_t* total) {
  if (type < PAT_LINEAR || type > PAT_RELU_NEGATIVE) return fail(LRP_ERR_INVALID, "unknown pattern type %d", type);
  LRP_TRY(pattern_mode_check());
  size_t max_kc = 0, max_cout = 0;
  for (const ConvLayer& L : layers) {
    max_kc = std::max(max_kc, (size_t)9 * L.cin * L.cout);
    max_cout = std::max(max_cout, (size_t)L.cout);
  }
  if ((size_t)27 * layers[0].cout * sizeof(float) > 65536)
    return fail(LRP_ERR_UNSUPPORTED, "the image layer's fit holds 27 x cout weights in LDS: cout <= 592");
  auto sum_bytes = [&](size_t li) { return PatternState::sum_doubles(layers[li].cin, layers[li].cout) * sizeof(double); };
  for (size_t li = 0; li < layers.size(); ++li) LRP_TRY(grow(pat.layer[li].sums, sum_bytes(li), total));
  LRP_TRY(grow(pat.prod, 2 * max_kc * sizeof(float), total));
  pat.ws_floats = 8 * max_kc;
  LRP_TRY(grow(pat.ws, pat.ws_floats * sizeof(float), total));
  LRP_TRY(grow(pat.part, (size_t)PAT_MAX_CHUNKS * 2 * max_cout * sizeof(double), total));
  LRP_TRY(alloc_keep_acts(total));
  LRP_HIP_CHECK(hipDeviceSynchronize());               // (an earlier fit's launches may still add to the sums)
  for (size_t li = 0; li < layers.size(); ++li) LRP_HIP_CHECK(hipMemset(pat.layer[li].sums.p, 0, sum_bytes(li)));
  LRP_HIP_CHECK(hipDeviceSynchronize());
  pat.type = type; pat.fit_epoch = -1; pat.batches = 0;   // (an open fit keeps the layer inputs: acts_wanted)
  encoded = 0;                                         // the next encode keeps the layer inputs
  return LRP_OK;
}
inline int Encoder::pattern_fit_check() const {
  LRP_TRY(pattern_mode_check());
  if (pat.type < 0) return fail(LRP_ERR_STATE, "lrp_pattern_fit_begin must be called first");
  return LRP_OK;
}
// the images of the last encode: per conv c = conv(x) + b, the mask pass, the two products, the float64 sums
inline int Encoder::pattern_fit_batch(hipStream_t st) {
  LRP_TRY(pattern_fit_check());
  LRP_TRY(encoded_ok("(after lrp_pattern_fit_begin) before lrp_pattern_fit_batch", keep_acts));
  if (pat.fit_epoch == encode_epoch) return fail(LRP_ERR_STATE, "this encode is already part of the fit: an encode is accumulated at most once");
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
    hipLaunchKernelGGL(pattern_mask_kernel, dim3(chunks), dim3(256), 0, st, c, L.bias.as<float>(), m, ym, pat.part.as<double>(), P, L.cout,
                       rows_per, pat.type);
    LRP_HIP_CHECK(hipGetLastError());
    prof.end(st, 0.0);
    SgemmArgs a{};                                     // X^T . rhs, all nine taps in one launch (the weight gradient's product)
    a.A = layer_input(li); a.lda = L.cin; a.ldb = L.cout; a.ldc = L.cout;
    a.M = L.cin; a.N = L.cout; a.K = P; a.transA = 1; a.transB = 0;
    a.gather = 1; a.gH = L.H; a.gW = L.W; a.taps = 9; a.tapC = (long)L.cin * L.cout;
    prof.begin(st);
    a.B = m; a.C = pat.prod.as<float>();
    LRP_HIP_CHECK(sgemm(a, pat.ws.as<float>(), pat.ws_floats, st));
    a.B = ym; a.C = pat.prod.as<float>() + KC;
    LRP_HIP_CHECK(sgemm(a, pat.ws.as<float>(), pat.ws_floats, st));
    prof.end(st, 4.0 * (double)P * (double)KC);
    prof.begin(st);
    hipLaunchKernelGGL(pattern_accumulate_kernel, dim3(stream_grid(2 * KC)), dim3(256), 0, st, pat.prod.as<float>(), pat.part.as<double>(), chunks,
                       pat.layer[li].sums.as<double>(), KC, L.cout, (double)P);
    LRP_HIP_CHECK(hipGetLastError());
    prof.end(st, 0.0);
  }
  pat.fit_epoch = encode_epoch;
  ++pat.batches;
  return LRP_OK;
}
inline int Encoder::pattern_alloc(int li) {
  return grow(pat.layer[li].A, (size_t)9 * layers[li].cin * layers[li].cout * sizeof(float), ws_total);
}
// sums -> patterns, installed; the fit is closed (its sums stay readable until the next lrp_pattern_fit_begin)
inline int Encoder::pattern_fit_end(hipStream_t st) {
  LRP_TRY(pattern_fit_check());
  if (pat.batches < 1) return fail(LRP_ERR_STATE, "lrp_pattern_fit_batch must run at least once before lrp_pattern_fit_end");
  for (size_t li = 0; li < layers.size(); ++li) LRP_TRY(pattern_alloc((int)li));
  for (size_t li = 0; li < layers.size(); ++li) {
    const ConvLayer& L = layers[li];
    PatternState::Layer& pl = pat.layer[li];
    const int CP = li == 0 ? 0 : conv_cinp(L.cin);
    hipLaunchKernelGGL(pattern_compute_kernel, dim3(L.cout), dim3(256), 0, st, pl.sums.as<double>(),
                       li == 0 ? L.w_fwd.as<float>() : L.w_fwd_a.as<float>(), li == 0 ? 64 : 9 * CP, CP, L.cin, L.cout, pl.A.as<float>());
    LRP_HIP_CHECK(hipGetLastError());
    pl.have = true;
    pl.packed = false;
  }
  pat.type = -1;                                       // (the caches of the last encode stay valid: they hold more than is needed)
  return LRP_OK;
}
inline int Encoder::pattern_set(int li, const float* A_dev, hipStream_t st) {
  PatternState::Layer& pl = pat.layer[li];
  LRP_TRY(pattern_alloc(li));
  LRP_HIP_CHECK(hipMemcpyAsync(pl.A.p, A_dev, (size_t)9 * layers[li].cin * layers[li].cout * sizeof(float), hipMemcpyDeviceToDevice, st));
  pl.have = true;
  pl.packed = false;
  return LRP_OK;
}
// the walk's matrices of every layer whose pattern or weights changed: A and A * w as the gradient walk's w_bwd_full is packed
inline int Encoder::pattern_pack(hipStream_t st) {
  for (size_t li = 0; li < layers.size(); ++li) {
    const ConvLayer& L = layers[li];
    PatternState::Layer& pl = pat.layer[li];
    if (pl.packed) continue;
    const size_t nb = li == 0 ? (size_t)conv_npad(IMG_T_COLS) * conv_cinp(L.cout) : (size_t)conv_npad(L.cin) * 9 * conv_cinp(L.cout);
    for (DevBuf* d : {&pl.bwd, &pl.bwd_w}) LRP_TRY(grow(*d, nb * sizeof(float), ws_total, 2, st));
    if (li == 0) {
      hipLaunchKernelGGL(pattern_pack_image_kernel, dim3((27 * L.cout + 255) / 256), dim3(256), 0, st, pl.A.as<float>(), pl.bwd.as<float>(),
                         L.cout, conv_cinp(L.cout));
    } else {
      const int CPo = conv_cinp(L.cout), Npb = conv_npad(L.cin);
      hipLaunchKernelGGL(pack_conv_dev_kernel, dim3(stream_grid(nb)), dim3(256), 0, st, pl.A.as<float>(), pl.bwd.as<float>(), 1, L.cin,
                         L.cout, CPo, Npb, 0, 0);
    }
    hipLaunchKernelGGL(pattern_mul_kernel, dim3(stream_grid(nb / 4)), dim3(256), 0, st, pl.bwd.as<f32x4>(), L.w_bwd_full.as<f32x4>(),
                       pl.bwd_w.as<f32x4>(), nb / 4);
    LRP_HIP_CHECK(hipGetLastError());
    pl.packed = true;
  }
  return LRP_OK;
}
inline int Encoder::pattern_walk_check(int n) const {
  LRP_TRY(tokens_ok(n));
  LRP_TRY(pattern_mode_check());
  for (size_t li = 0; li < layers.size(); ++li)
    if (!pat.layer[li].have)
      return fail(LRP_ERR_STATE, "conv '%s' has no pattern: fit them (lrp_pattern_fit_*) or set them (lrp_set_patterns)", layers[li].name.c_str());
  return encoded_ok("before the pattern walk");
}
// a row's divisor: max |x| of each of the n rows of x, 1 where that is 0
inline int Encoder::pattern_row_div(const float* x, int n, size_t per_row, hipStream_t st) {
  const int chunks = pattern_chunks(per_row);
  hipLaunchKernelGGL(pattern_absmax_part_kernel, dim3(chunks, n), dim3(256), 0, st, x, per_row, pat.maxpart.as<float>());
  hipLaunchKernelGGL(pattern_absmax_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, pat.maxpart.as<float>(), n, chunks, pat.div.as<float>());
  return launched();
}
inline int Encoder::explain_pattern(int n, const int* row2img_dev, const float* head_dev, float* R_img_dev, bool attribution, hipStream_t st) {
  LRP_TRY(pattern_walk_check(n));
  LRP_TRY(wait_gates(st));
  const int nl = (int)layers.size();
  float *S = s0.as<float>(), *Snext = s1.as<float>();
  auto conv_args = [&](int li) {
    const ConvLayer& L = layers[li];
    ConvArgs ca = conv3x3_args(L, n, S, L.cout);
    ca.wpk = (attribution ? pat.layer[li].bwd_w : pat.layer[li].bwd).as<float>(); ca.row2img = row2img_dev;
    if (li > 0) { ca.N = L.cin; ca.out = Snext; ca.gate_none = 1; ca.out_plain = 1; }
    return ca;
  };
  LRP_TRY(plan_or_refuse(nl - 1, -1, n, PREC_FP32, conv_args, [&](int li) {
    return fail(LRP_ERR_UNSUPPORTED, "conv %d: no exact-fp32 launch reads %d channels into a plain accumulator", li, layers[li].cout);
  }));
  const size_t img_row = (size_t)img_h * img_w * 3;
  if (!pat.div.p) {
    int max_chunks = std::max(pattern_chunks(layers.back().act_elems()), pattern_chunks(img_row));
    for (int li = 1; li < nl; ++li) max_chunks = std::max(max_chunks, pattern_chunks((size_t)layers[li].H * layers[li].W * layers[li].cin));
    LRP_TRY(pat.div.alloc((size_t)max_tokens * sizeof(float), ws_total));
    LRP_TRY(pat.maxpart.alloc((size_t)max_tokens * max_chunks * sizeof(float), ws_total));
  }
  LRP_TRY(pattern_pack(st));
  const float* div = pat.project ? pat.div.as<float>() : nullptr;
  const size_t top_row = layers.back().act_elems();    // the head, projected, through the top ReLU
  prof.begin(st);
  if (pat.project) LRP_TRY(pattern_row_div(head_dev, n, top_row, st));
  hipLaunchKernelGGL(pattern_head_kernel, dim3(stream_grid((size_t)n * top_row / 4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(head_dev),
                     feat.as<f32x4>(), row2img_dev, div, reinterpret_cast<f32x4*>(S), n, top_row / 4);
  LRP_HIP_CHECK(hipGetLastError());
  prof.end(st, 0.0);
  for (int li = nl - 1; li >= 1; --li) {
    const ConvLayer &L = layers[li], &P = layers[li - 1];
    LRP_TRY(timed_conv(EPI_MUL, conv_args(li), st, PREC_FP32, layer_flop(n, li)));
    if (P.pool_after) LRP_TRY(full_gate(li - 1, st));
    PatternProjectArgs t{};
    t.acc = Snext; t.gate = P.G.as<float>(); t.row2img = row2img_dev; t.div = div; t.S = S;
    t.n = n; t.H = L.H; t.W = L.W; t.C = L.cin;
    prof.begin(st);
    if (pat.project) LRP_TRY(pattern_row_div(Snext, n, (size_t)L.H * L.W * L.cin, st));
    const dim3 grid(stream_grid((size_t)n * L.H * L.W * (L.cin / 4)));
    if (P.pool_after) hipLaunchKernelGGL((pattern_project_kernel<true>), grid, dim3(256), 0, st, t);
    else hipLaunchKernelGGL((pattern_project_kernel<false>), grid, dim3(256), 0, st, t);
    LRP_HIP_CHECK(hipGetLastError());
    prof.end(st, 0.0);
  }
  LRP_TRY(image_layer_step(conv_args(0), n, PREC_FP32, layer_flop(n, 0), Snext, R_img_dev, 1, 0.f, 0.f, st));
  if (pat.project) {
    prof.begin(st);
    LRP_TRY(pattern_row_div(R_img_dev, n, img_row, st));
    hipLaunchKernelGGL(pattern_scale_kernel, dim3(stream_grid((size_t)n * img_row / 4)), dim3(256), 0, st, R_img_dev, img_row, pat.div.as<float>(), n);
    LRP_HIP_CHECK(hipGetLastError());
    prof.end(st, 0.0);
  }
  return LRP_OK;
}
}  // namespace lrp
