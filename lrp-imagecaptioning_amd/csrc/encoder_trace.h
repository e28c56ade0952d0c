// encoder_trace.h — the layer trace of the VGG walk (lrp_set_layer_trace, lrp_cnn_explain_traced; trace_kernels.h
// has the arithmetic).  State: TraceState (encoder_state.h), Encoder::tr.
// The reversed tensors of the reference's reverse analyzers: the head, and the relevance at the input of every node (conv or 2x2
// pool, in execution order).  While the switch is on the handle is one more user of keep_acts; nothing else changes, and what the
// traced walk needs beyond the rule's own buffers (the partials of its reductions) appears with the first traced call.  The walk
// runs under the handle's rule, the default one or a table (encoder_rules.h).  Included by encoder.h behind struct Encoder.
#pragma once
namespace lrp {
// in sorted-id order: (-1, 0) the head, (0, 0) the image, ...
inline std::vector<TraceTensor> Encoder::trace_tensors() const {
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
inline int Encoder::trace_index_of_conv(int li) const {
  int t = 1;
  for (int q = 0; q < li; ++q) t += layers[q].pool_after ? 2 : 1;
  return t;
}
// where the tensors `mask` selects lie in a keep buffer for n rows (floats; every tensor starts on a multiple of 4): -1 for the
// others.  Returns the buffer's size.
inline int64_t Encoder::trace_keep_layout(int n, uint64_t mask, std::vector<int64_t>& off) const {
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
inline int Encoder::set_layer_trace(bool on, int64_t* total) {
  if (on == tr.on) return LRP_OK;                      // the same setting again changes nothing
  if (on) LRP_TRY(alloc_keep_acts(total));
  tr.on = on;
  encoded = 0;                                         // the next encode keeps (or stops keeping) the layer inputs
  return LRP_OK;
}
inline int Encoder::trace_check(int n) const {
  LRP_TRY(tokens_ok(n));
  if (walk_f16) return fail(LRP_ERR_UNSUPPORTED, "LRP_PREC_F16X2 has no traced walk (its chains travel under per-token scales)");
  if (table_on() && !table_runs()) return fail(LRP_ERR_UNSUPPORTED, "epsilon rules run in LRP_PREC_FP32 only");
  if (!tr.on) return fail(LRP_ERR_STATE, "lrp_set_layer_trace(h, 1) must be called before lrp_cnn_explain_traced");
  return encoded_ok("(after lrp_set_layer_trace) before lrp_cnn_explain_traced");
}
inline int Encoder::trace_chunks(const ConvLayer& L, bool split) {
  const size_t items = (size_t)L.H * L.W * (L.cin / (split ? 8 : 4));
  return (int)((items + TRACE_ITEMS_PER_BLOCK - 1) / TRACE_ITEMS_PER_BLOCK);
}
inline int Encoder::tensor_stats(const float* x, int rows, size_t per_row, double* stats, hipStream_t st) {
  hipLaunchKernelGGL(tensor_stats_kernel, dim3(rows), dim3(1024), 0, st, x, per_row, stats);
  return launched();
}
inline int Encoder::trace_layer(bool pool, bool split, int k, const TraceLayerArgs& t, int nblk, hipStream_t st) {
  const dim3 grid(nblk, t.n);
#define LRP_TRACE_CASE(P, S, K) \
if (pool == P && split == S && k == K) hipLaunchKernelGGL((trace_layer_kernel<P, S, K>), grid, dim3(256), 0, st, t)
  LRP_TRACE_CASE(false, false, 1); LRP_TRACE_CASE(false, false, 2); LRP_TRACE_CASE(false, true, 1); LRP_TRACE_CASE(false, true, 2);
  LRP_TRACE_CASE(true, false, 1); LRP_TRACE_CASE(true, false, 2); LRP_TRACE_CASE(true, true, 1); LRP_TRACE_CASE(true, true, 2);
#undef LRP_TRACE_CASE
  return launched();
}
// stats_dev (n_tensors, n, 4) float64; keep_dev with `keep_off` from trace_keep_layout (nullptr: nothing is kept)
inline int Encoder::explain_traced(int n, const int* row2img_dev, const float* R_feat_dev, float* R_img_dev, double* stats_dev, float* keep_dev,
                   const std::vector<int64_t>& keep_off, hipStream_t st) {
  LRP_TRY(trace_check(n));
  LRP_TRY(wait_gates(st));
  const bool split = table_split();                    // (no table: the handle's mode alone, as the default walk)
  const int rp = split ? PREC_BF16X3 : PREC_FP32, nl = (int)layers.size();
  float *S, *Snext;
  chain_buffers(RuleTableState::chains_of(rules.table) == 2, S, Snext);
  const ConvRule& r0 = rule_at(0);
  auto conv_args = [&](int li) {                       // li >= 1: into a plain accumulator, the gates are trace_layer_kernel's
    const ConvLayer& L = layers[li];
    ConvArgs ca = conv3x3_args(L, n, S, rule_at(li).chains() * L.cout);
    ca.wpk = rule_matrix(li, split); ca.row2img = row2img_dev;
    if (li > 0) { ca.N = L.cin; ca.out = Snext; ca.gate_none = 1; ca.out_plain = 1; }
    return ca;
  };
  LRP_TRY(plan_or_refuse(nl - 1, -1, n, rp, conv_args, [&](int li) {
    return fail(LRP_ERR_UNSUPPORTED, "conv %d: no launch reads %d chain(s) of %d channels into a plain accumulator", li, rule_at(li).chains(),
                layers[li].cout);
  }));
  int max_chunks = 1;                                  // (sized for either arithmetic: it never grows)
  for (int li = 1; li < nl; ++li) max_chunks = std::max(max_chunks, trace_chunks(layers[li], false));
  const size_t part_row = (size_t)max_chunks * TRACE_PART, part_tensor = (size_t)max_tokens * part_row;
  if (!tr.part.p) LRP_TRY(tr.part.alloc(2 * part_tensor * sizeof(double), ws_total));
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
    LRP_TRY(timed_conv(EPI_MUL, conv_args(li), st, rp, (double)rule_at(li).chains() * layer_flop(n, li)));
    if (P.pool_after) LRP_TRY(full_gate(li - 1, st));
    const int tc = trace_index_of_conv(li), nblk = trace_chunks(L, split);
    TraceLayerArgs t{};
    t.acc = Snext; t.a = layer_input(li); t.gpos = P.pool_after ? P.G.as<float>() : nullptr;
    t.g0 = table_on() ? table_gate(li - 1) : P.G.as<float>(); t.g1 = k == 2 ? rules.layer[li - 1].Gn.as<float>() : nullptr;
    t.row2img = row2img_dev; t.S = S;
    t.keep_conv = keep_ptr(tc); t.keep_pool = P.pool_after ? keep_ptr(tc - 1) : nullptr;
    t.part_conv = tr.part.as<double>(); t.part_pool = tr.part.as<double>() + part_tensor;
    t.n = n; t.H = L.H; t.W = L.W; t.C = L.cin;
    prof.begin(st);
    LRP_TRY(trace_layer(P.pool_after, split, k, t, nblk, st));
    prof.end(st, 0.0);
    hipLaunchKernelGGL(trace_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, t.part_conv, n, nblk, stats_of(tc));
    if (P.pool_after) hipLaunchKernelGGL(trace_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, t.part_pool, n, nblk, stats_of(tc - 1));
    LRP_HIP_CHECK(hipGetLastError());
  }
  LRP_TRY(image_layer_step(conv_args(0), n, rp, (double)r0.chains() * layer_flop(n, 0), Snext, R_img_dev, r0.img_mode(), r0.low, r0.high, st));
  return whole(1, R_img_dev);
}
}  // namespace lrp
