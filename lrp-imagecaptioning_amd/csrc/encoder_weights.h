// encoder_weights.h — the device packers of Encoder.  Every operand copy is built ON THE DEVICE from the HWIO array in HBM:
// lrp_set_weight (the caller's host array is copied there first), lrp_set_weight_dev (the multi-GPU start-up path: the bundle
// arrives over RCCL/xGMI and never visits the host) and the fine-tune step (weights change every iteration).  "<name>_W" is split
// by sign (RR:256-260).  The analyzers' own copies (the table's matrices, A * w of the patterns) are marked stale here and rebuilt
// by their role headers.  Included by encoder.h behind struct Encoder.
#pragma once
namespace lrp {
inline int Encoder::alloc_conv_operands(int li, int64_t* total, hipStream_t st) {
  ConvLayer& L = layers[li];
  auto mk = [&](DevBuf& d, size_t floats) { return grow(d, floats * sizeof(float), total, 2, st); };   // (a layer's sizes never change)
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
inline int Encoder::repack_conv_weight_from_device(int li, const float* w_dev, float* tmp, hipStream_t st) {
  ConvLayer& L = layers[li];
  if (li == 0) {
    const int Npb = conv_npad(IMG_T_COLS), Kb = conv_cinp(L.cout);
    hipLaunchKernelGGL(pack_image_layer_dev_kernel, dim3((27 * L.cout + 255) / 256), dim3(256), 0, st, w_dev, L.w_fwd.as<float>(),
                       L.w_bwd.as<float>(), L.w_bwd_full.as<float>(), L.cout, Kb);
    const size_t nb = (size_t)Npb * Kb;
    if (L.w_fwd_il.p) {
      hipLaunchKernelGGL(dual_interleave_rows_kernel, dim3(stream_grid((size_t)2 * L.cout * 64)), dim3(256), 0, st, L.w_fwd.as<float>(),
                         L.w_fwd_il.as<float>(), L.cout, 64);
      LRP_TRY(make_f16_operand(f16_slots, L.w_fwd_il.as<float>(), (size_t)conv_npad(2 * L.cout) * 64, 0, 0, L.w_fwd_h, L.wds, nullptr, st));
    }
    hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(nb / 8)), dim3(256), 0, st, L.w_bwd.as<float>(), L.w_bwd_s.as<float>(), nb / 8);
    LRP_TRY(make_f16_operand(f16_slots, L.w_bwd.as<float>(), nb, 0, 0, L.w_bwd_h, L.wbs, nullptr, st));
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
  LRP_TRY(make_f16_operand(f16_slots, L.w_fwd_il.p ? L.w_fwd_il.as<float>() : L.w_fwd.as<float>(), (size_t)Np2 * 9 * CPi, 0, 0, L.w_fwd_h,
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
  LRP_TRY(make_f16_operand(f16_slots, L.w_bwd.as<float>(), nb, Npb, 9 * CPo, L.w_bwd_h, L.wbs, nullptr, st));
  if (L.w_bwd_frag_h.p)
    hipLaunchKernelGGL(pack_frag_dev_kernel, dim3(stream_grid((size_t)CPo / 32 * 9 * 512)), dim3(256), 0, st, L.w_bwd_h.as<float>(),
                       L.w_bwd_frag_h.as<float>(), CPo, 64);
  pack(L.w_bwd_full.as<float>(), 1, Npb, 0, 0);
  split(L.w_bwd_full.as<float>(), L.w_bwd_full_s.as<float>(), nb);
  LRP_HIP_CHECK(hipGetLastError());
  return LRP_OK;
}
// fine-tune step: layer li (weights and bias) from the trainer's master buffer
inline int Encoder::repack_conv_from_device(int li, const float* w_dev, const float* b_dev, float* tmp, hipStream_t st) {
  ConvLayer& L = layers[li];
  if (!L.have_w || !L.have_b) return fail(LRP_ERR_STATE, "layer %d has no operand copies to rebuild", li);
  LRP_TRY(repack_conv_weight_from_device(li, w_dev, tmp, st));
  analyzers_stale(li);
  if (table_on()) LRP_TRY(pack_table_layer(li, w_dev, st));
  L.norm_dirty = true;
  LRP_HIP_CHECK(hipMemcpyAsync(L.bias.p, b_dev, (size_t)L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
  L.raw_w_dev.release(); L.raw_b_dev.release();   // stale from here on (the trainer's master buffer is the truth)
  return LRP_OK;
}
// lrp_set_weight / lrp_set_weight_dev: "<name>_W" / "<name>_b" from host or device memory (`kind`) — one copy into
// HBM, then the device packers; nothing here waits for the stream
inline int Encoder::set_conv_weight_dev(int li, const float* w, hipMemcpyKind kind, int64_t* total, hipStream_t st) {
  ConvLayer& L = layers[li];
  const size_t nW = (size_t)9 * L.cin * L.cout;
  LRP_TRY(wait_gates(st, true));                     // the side stream may still read the operand copies we replace
  analyzers_stale(li);
  if (!L.raw_w_dev.p) LRP_TRY(L.raw_w_dev.alloc(nW * sizeof(float), total));
  LRP_HIP_CHECK(hipMemcpyAsync(L.raw_w_dev.p, w, nW * sizeof(float), kind, st));
  LRP_TRY(alloc_conv_operands(li, total, st));
  LRP_TRY(repack_conv_weight_from_device(li, L.raw_w_dev.as<float>(), pack_tmp.as<float>(), st));
  L.have_w = true;
  L.norm_dirty = true;
  encoded = 0;                                      // caches belong to the old weights
  return LRP_OK;
}
inline int Encoder::set_conv_bias_dev(int li, const float* b, hipMemcpyKind kind, int64_t* total, hipStream_t st) {
  ConvLayer& L = layers[li];
  if (!L.raw_b_dev.p) LRP_TRY(L.raw_b_dev.alloc((size_t)L.cout * sizeof(float), total));
  if (!L.bias.p) LRP_TRY(L.bias.alloc((size_t)L.cout * sizeof(float), total));
  LRP_HIP_CHECK(hipMemcpyAsync(L.raw_b_dev.p, b, (size_t)L.cout * sizeof(float), kind, st));
  LRP_HIP_CHECK(hipMemcpyAsync(L.bias.p, L.raw_b_dev.p, (size_t)L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
  L.have_b = true;
  L.norm_dirty = true;
  dl.ref_stale = true;
  encoded = 0;
  return LRP_OK;
}
}  // namespace lrp
