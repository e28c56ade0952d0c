// encoder_deeplift.h — DeepLIFT for the VGG encoder (lrp_set_deeplift_reference, LRP_WALK_DEEPLIFT; DESIGN 4.20;
// deeplift_kernels.h has the rule).  State: DeepLiftState (encoder_state.h), Encoder::dl.
// One reference image per handle.  At encode, in LRP_PREC_FP32: the reference goes through forward_exact as a batch of one (the
// SAME path as the images: where image and reference agree on a receptive field Y and Yr are the same bits, which the dY == 0
// branch of SafeDivide needs) whenever weights, precision or reference changed, keeping Xr_l / Yr_l; behind the images' own
// forward dl_pass writes the gate D_l of every layer.  dX is not stored: the walk recomputes it from the kept layer inputs and
// Xr_l (the same 4 bytes read per element and token as a stored dX, and no (images x activations) tensor per layer; Xr_l is one
// image's worth and stays in L2).  dl_combine / dl_final are static: lrp_op_deeplift_conv (engine.hip) launches them too.
// The walk (explain_deeplift).  Per layer: the transposed conv with the full w (w_bwd_full, exact fp32, no gate in its epilogue)
// over the stacked chains [t ; g] — 2n rows, n in mode 1 — then dl_combine_kernel: the select, the 2x routing through a pool and
// both gates of the layer below.  The image layer is the stand-alone image launch over the same rows, then the select.
// Included by encoder.h behind struct Encoder.
#pragma once
namespace lrp {
inline int Encoder::set_deeplift_reference(const float* ref_host, float ref_scalar, int mode, int64_t* total) {
  if (mode == 0) {
    if (dl.mode != 0) { dl.mode = 0; encoded = 0; }    // (the buffers stay, idle)
    return LRP_OK;
  }
  const size_t img_elems = (size_t)img_h * img_w * 3;
  std::vector<float> ref(img_elems, ref_scalar);
  if (ref_host) ref.assign(ref_host, ref_host + img_elems);
  for (float v : ref)
    if (!(fabsf(v) < 3.0e38f)) return fail(LRP_ERR_INVALID, "the DeepLIFT reference must be finite");
  if (mode == dl.mode && ref == dl.ref_host) return LRP_OK;   // the same setting again changes nothing
  const size_t B = (size_t)max_images, NT = (size_t)max_tokens;
  for (size_t li = 0; li < layers.size(); ++li) {      // allocated by the first reference that is set
    const ConvLayer& L = layers[li];
    LRP_TRY(grow(dl.layer[li].Xr, (size_t)L.H * L.W * L.cin * sizeof(float), total));
    LRP_TRY(grow(dl.layer[li].Yr, L.act_elems() * sizeof(float), total));
    LRP_TRY(grow(dl.layer[li].Dl, B * L.act_elems() * sizeof(float), total));
  }
  if (mode == 2) {                                     // (one chain: the default walk's ping-pong s0 / s1)
    const size_t tok = std::max(max_act_elems(), img_elems / 3 * IMG_T_COLS);
    LRP_TRY(grow(dl.s0, 2 * NT * tok * sizeof(float), total));
    LRP_TRY(grow(dl.s1, 2 * NT * tok * sizeof(float), total));
    LRP_TRY(grow(dl.r2i, 2 * NT * sizeof(int), total));
  }
  LRP_TRY(alloc_keep_acts(total));
  LRP_HIP_CHECK(hipDeviceSynchronize());               // a walk in flight may still read the old reference
  LRP_HIP_CHECK(hipMemcpy(dl.layer[0].Xr.p, ref.data(), img_elems * sizeof(float), hipMemcpyHostToDevice));
  dl.ref_host.swap(ref);
  dl.mode = mode;
  dl.ref_stale = true;
  encoded = 0;                                         // the caches belong to the old reference
  return LRP_OK;
}
// the reference's forward: image slot 0 and every cache it touches are overwritten by the encode that follows
inline int Encoder::dl_reference_pass(hipStream_t st) {
  LRP_TRY(wait_gates(st, true));
  LRP_HIP_CHECK(hipMemcpyAsync(images.p, dl.layer[0].Xr.p, (size_t)img_h * img_w * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
  dl.capture = true;
  const int rc = forward_exact(1, st);
  dl.capture = false;
  LRP_TRY(rc);
  dl.ref_stale = false;
  return LRP_OK;
}
// behind the images' forward (keep_acts: every conv's input and activation is still there): the gates
inline int Encoder::dl_pass(int B, hipStream_t st) {
  for (size_t li = 0; li < layers.size(); ++li) {
    const ConvLayer& L = layers[li];
    const bool top = li + 1 == layers.size();
    const size_t n4 = (size_t)B * L.act_elems() / 4;
    if (L.pool_after) LRP_TRY(full_gate((int)li, st));
    const float* y = top ? feat.as<float>() : L.Akeep.as<float>();
    hipLaunchKernelGGL(dl_gate_kernel, dim3(stream_grid(n4)), dim3(256), 0, st, L.pool_after ? (const float*)nullptr : y,
                       L.pool_after ? L.G.as<float>() : (const float*)nullptr, L.pool_after ? L.P.as<float>() : (const float*)nullptr,
                       dl.layer[li].Yr.as<float>(), dl.layer[li].Dl.as<float>(), B, L.H, L.W, L.cout);
    LRP_HIP_CHECK(hipGetLastError());
  }
  dl.epoch = encode_epoch;
  return LRP_OK;
}
inline int Encoder::dl_combine(bool two, bool pool, const float* c, const float* x, const float* xr, const float* dn, const int* r2i, float* out, int n,
                      int H, int W, int C, hipStream_t st) {
  const dim3 grid(stream_grid((size_t)n * H * W * (C / 4)));
  if (two && pool) hipLaunchKernelGGL((dl_combine_kernel<true, true>), grid, dim3(256), 0, st, c, x, xr, dn, r2i, out, n, H, W, C);
  else if (two) hipLaunchKernelGGL((dl_combine_kernel<true, false>), grid, dim3(256), 0, st, c, x, xr, dn, r2i, out, n, H, W, C);
  else if (pool) hipLaunchKernelGGL((dl_combine_kernel<false, true>), grid, dim3(256), 0, st, c, x, xr, dn, r2i, out, n, H, W, C);
  else hipLaunchKernelGGL((dl_combine_kernel<false, false>), grid, dim3(256), 0, st, c, x, xr, dn, r2i, out, n, H, W, C);
  return launched();
}
inline int Encoder::dl_final(bool two, const float* c, const float* x, const float* xr, const int* r2i, float* out, int n, size_t per, hipStream_t st) {
  const bool v4 = !(per & 3);
  const dim3 grid(stream_grid((size_t)n * per / (v4 ? 4 : 1)));
  if (two && v4) hipLaunchKernelGGL((dl_final_kernel<true, 4>), grid, dim3(256), 0, st, c, x, xr, r2i, out, n, per);
  else if (two) hipLaunchKernelGGL((dl_final_kernel<true, 1>), grid, dim3(256), 0, st, c, x, xr, r2i, out, n, per);
  else if (v4) hipLaunchKernelGGL((dl_final_kernel<false, 4>), grid, dim3(256), 0, st, c, x, xr, r2i, out, n, per);
  else hipLaunchKernelGGL((dl_final_kernel<false, 1>), grid, dim3(256), 0, st, c, x, xr, r2i, out, n, per);
  return launched();
}
inline int Encoder::dl_check(int n) const {
  LRP_TRY(tokens_ok(n));
  if (prec != PREC_FP32)
    return fail(LRP_ERR_UNSUPPORTED, "the DeepLIFT walk runs in LRP_PREC_FP32 only (dY of fp16-pair activations means nothing where it is small): "
                                     "set it with lrp_set_precision and call lrp_encode_images again");
  if (dl.mode == 0) return fail(LRP_ERR_STATE, "lrp_set_deeplift_reference must be called before the DeepLIFT walk");
  return encoded_ok("(after lrp_set_deeplift_reference) before the DeepLIFT walk", dl.epoch == encode_epoch);
}
inline int Encoder::explain_deeplift(int n, const int* row2img_dev, const float* head_dev, float* R_img_dev, hipStream_t st) {
  LRP_TRY(dl_check(n));
  LRP_TRY(wait_gates(st));
  const bool two = dl.mode == 2;
  const int rows = two ? 2 * n : n, nl = (int)layers.size();
  const double chains = two ? 2.0 : 1.0;
  float *S = (two ? dl.s0 : s0).as<float>(), *Snext = (two ? dl.s1 : s1).as<float>();
  const int* r2i_rows = two ? dl.r2i.as<int>() : row2img_dev;     // row2img, twice for the two chains' rows
  auto conv_args = [&](int li) {
    const ConvLayer& L = layers[li];
    ConvArgs ca = conv3x3_args(L, rows, S, L.cout);
    ca.wpk = L.w_bwd_full.as<float>();
    if (li == 0) ca.row2img = r2i_rows;
    else { ca.N = L.cin; ca.out = Snext; ca.gate_none = 1; }
    return ca;
  };
  LRP_TRY(plan_or_refuse(nl - 1, -1, rows, PREC_FP32, conv_args, [&](int li) {
    return fail(LRP_ERR_UNSUPPORTED, "conv %d: no exact-fp32 launch for %d rows of %d channels", li, rows, layers[li].cout);
  }));
  if (two) {
    LRP_HIP_CHECK(hipMemcpyAsync(dl.r2i.p, row2img_dev, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
    LRP_HIP_CHECK(hipMemcpyAsync(dl.r2i.as<int>() + n, row2img_dev, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
  }
  const ConvLayer& T = layers.back();                  // the head through the top layer's gates
  prof.begin(st);
  LRP_TRY(dl_combine(two, false, head_dev, nullptr, nullptr, dl.layer[nl - 1].Dl.as<float>(), row2img_dev, S, n, T.H, T.W, T.cout, st));
  prof.end(st, 0.0);
  for (int li = nl - 1; li >= 1; --li) {
    const ConvLayer& L = layers[li];
    LRP_TRY(timed_conv(EPI_MUL, conv_args(li), st, PREC_FP32, chains * layer_flop(n, li)));
    prof.begin(st);
    LRP_TRY(dl_combine(two, layers[li - 1].pool_after, Snext, layer_input(li), dl.layer[li].Xr.as<float>(), dl.layer[li - 1].Dl.as<float>(), row2img_dev,
                       S, n, L.H, L.W, L.cin, st));
    prof.end(st, 0.0);
  }
  float* c = img_fused() ? Snext : S;                  // (LRP_IMG_FUSED=0: the tap GEMM into Snext, its stencil back into S)
  LRP_TRY(image_layer_step(conv_args(0), rows, PREC_FP32, chains * layer_flop(n, 0), Snext, c, 1, 0.f, 0.f, st));
  prof.begin(st);
  LRP_TRY(dl_final(two, c, images.as<float>(), dl.layer[0].Xr.as<float>(), row2img_dev, R_img_dev, n, (size_t)img_h * img_w * 3, st));
  prof.end(st, 0.0);
  return LRP_OK;
}
}  // namespace lrp
