// engine.hip — the C ABI of liblrp_hip.so (include/lrp_hip.h).  Thin glue: argument
// checks, host->device staging of the small index arrays, and dispatch into the
// encoder (CNN half) and decoder (LSTM/attention half) orchestration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <exception>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "augment_kernels.h"
#include "common.h"
#include "conv_launch.h"
#include "conv_plan.h"
#include "conv_sparse.h"
#include "decoder.h"
#include "encoder.h"
#include "eval_kernels.h"
#include "gradcam_kernels.h"
#include "cam_kernels.h"     // (after gradcam_kernels.h: it shares that kernel's stages)
#include "perturb_kernels.h"
#include "resnet_encoder.h"
#include "rules_kernels.h"
#include "saliency_kernels.h"
#include "score_kernels.h"
#include "segment_kernels.h"
#include "trainer.h"

namespace lrp {
std::string& last_error_ref() {
  static thread_local std::string e;
  return e;
}
}  // namespace lrp

using namespace lrp;

struct lrp_handle {
  lrp_config cfg;
  int64_t ws_bytes = 0;
  Encoder enc;             // VGG-style encoder (LRP_ENC_VGG)
  ResNetEncoder rn;        // ResNet bottleneck encoder (LRP_ENC_RESNET)
  bool resnet = false;
  Decoder dec;
  Trainer trainer;         // fine-tune step (lrp_train_*), VGG + adaptive attention
  float* feat() { return resnet ? rn.feat.as<float>() : enc.feat.as<float>(); }
  int& encoded() { return resnet ? rn.encoded : enc.encoded; }
  bool& features_only() { return resnet ? rn.features_only : enc.features_only; }
  DevBuf idx_dev;          // staged (img_idx | t) for the current explain call
  DevBuf rfeat_tmp;        // R_feat when the caller does not want it back
  int* idx_pinned = nullptr;
  hipEvent_t ev_idx = nullptr;   // the last H2D copy out of idx_pinned (guards its reuse without a stream sync)
  ~lrp_handle() {
    if (ev_idx) { (void)hipEventSynchronize(ev_idx); (void)hipEventDestroy(ev_idx); }
    if (idx_pinned) (void)hipHostFree(idx_pinned);
  }
};

static hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---- the two invariants of the boundary (include/lrp_hip.h:10-20), enforced in ONE place for every entry point:
//  (1) no C++ exception crosses the C ABI: bodies run inside guarded(), which maps std::bad_alloc -> LRP_ERR_NOMEM and
//      anything else -> LRP_ERR_INVALID (std::vector / std::string / std::map in the weight setters, the decoder and
//      the evaluation entries can throw; `new lrp_handle` too);
//  (2) a handle's work runs on the handle's device: with_handle() makes cfg.device current for the duration of the call
//      and restores the caller's device on return (lazy allocations — Decoder::finalize, the scan / gradient packs, the
//      trainer's buffers — and every kernel launch would otherwise land on whatever device the calling thread had
//      current: a process that drives several GPUs must not have to remember a hipSetDevice per call).
static int fail_nothrow(int code, const char* msg) noexcept {
  try { last_error_ref() = msg ? msg : ""; } catch (...) {}
  return code;
}
template <class F>
static int guarded(F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail_nothrow(LRP_ERR_NOMEM, "out of host memory inside liblrp_hip");
  } catch (const std::exception& e) {
    return fail_nothrow(LRP_ERR_INVALID, e.what());
  } catch (...) {
    return fail_nothrow(LRP_ERR_INVALID, "unknown C++ exception inside liblrp_hip");
  }
}
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) {
      err = hipSetDevice(dev);
      switched = err == hipSuccess;
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};
template <class F>
static int with_handle(const lrp_handle* h, F&& body) noexcept {
  return guarded([&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    DeviceGuard g(h->cfg.device);
    if (g.err != hipSuccess) return fail(LRP_ERR_HIP, "cannot make device %d current: %s", h->cfg.device, hipGetErrorString(g.err));
    return body();
  });
}

extern "C" {

int lrp_abi_version(void) { return LRP_ABI_VERSION; }
int lrp_reload_switches(void) {
  return guarded([&]() -> int { lrp::sw().load(); return LRP_OK; });
}

int lrp_conv_plan(int32_t epi, int32_t prec, int32_t terms, int32_t NB, int32_t H, int32_t W, int32_t N, int32_t Cin, int32_t taps,
                  int32_t split, uint32_t flags, int32_t* out11) {
  return guarded([&]() -> int {
    static_assert(LRP_EPI_BIAS_RELU == lrp::EPI_BIAS_RELU && LRP_EPI_BIAS == lrp::EPI_BIAS && LRP_EPI_MUL == lrp::EPI_MUL &&
                  LRP_EPI_MUL_UP2 == lrp::EPI_MUL_UP2 && LRP_EPI_FWD_DUAL == lrp::EPI_FWD_DUAL && LRP_EPI_STORE == lrp::EPI_STORE &&
                  LRP_EPI_IMG_STENCIL == lrp::EPI_IMG_STENCIL, "lrp_hip.h LRP_EPI_*");
    static_assert(LRP_OPND_FP32 == lrp::PREC_FP32 && LRP_OPND_BF16X3 == lrp::PREC_BF16X3 && LRP_OPND_F16X2 == lrp::PREC_F16X2, "lrp_hip.h LRP_OPND_*");
    static_assert(LRP_FORM_PLAIN == lrp::FORM_PLAIN && LRP_FORM_SMALL == lrp::FORM_SMALL && LRP_FORM_HALO == lrp::FORM_HALO &&
                  LRP_FORM_BREG == lrp::FORM_BREG && LRP_FORM_POOL == lrp::FORM_POOL && LRP_FORM_IMG == lrp::FORM_IMG && LRP_FORM_BREG8 == lrp::FORM_BREG8 &&
                  LRP_FORM_BREG4 == lrp::FORM_BREG4 && LRP_FORM_BREG4_POOL == lrp::FORM_BREG4_POOL, "lrp_hip.h LRP_FORM_*");
    if (!out11) return fail(LRP_ERR_INVALID, "null argument");
    lrp::ConvAsk q;
    q.epi = epi; q.prec = prec; q.terms = terms; q.NB = NB; q.H = H; q.W = W; q.N = N; q.Cin = Cin; q.taps = taps; q.split = split;
    q.frag = flags & LRP_PLAN_FRAG; q.join = flags & LRP_PLAN_JOIN; q.dual_il = flags & LRP_PLAN_DUAL_IL; q.gmask = flags & LRP_PLAN_GMASK;
    q.up2_src = flags & LRP_PLAN_UP2_SRC; q.img_part = flags & LRP_PLAN_IMG_PART; q.pool_gc = flags & LRP_PLAN_POOL_GC;
    q.dual_mul = flags & LRP_PLAN_DUAL_MUL;
    const lrp::ConvPlan p = lrp::conv_plan(q);
    const int v[11] = {p.ok ? 1 : 0, p.form, p.BM, p.BN, p.threads, p.tw, p.th, p.hrows, p.tpt, p.m_tiles, p.n_tiles};
    for (int i = 0; i < 11; ++i) out11[i] = v[i];
    return LRP_OK;
  });
}

int64_t lrp_launch_count(void) { return (int64_t)lrp::g_launch_count.load(std::memory_order_relaxed); }
const char* lrp_last_error(void) { return last_error_ref().c_str(); }

int lrp_create(const lrp_config* cfg, lrp_handle** out) {
  return guarded([&]() -> int {
    if (!cfg || !out) return fail(LRP_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->abi_version != LRP_ABI_VERSION) return fail(LRP_ERR_INVALID, "abi_version %d != %d", cfg->abi_version, LRP_ABI_VERSION);
    if (cfg->decoder != LRP_DEC_ADAPTIVE && cfg->decoder != LRP_DEC_GRIDTD)
      return fail(LRP_ERR_UNSUPPORTED, "unknown decoder kind %d", cfg->decoder);
    if (cfg->max_images < 1 || cfg->max_tokens < 1 || cfg->max_caption_len < 2)
      return fail(LRP_ERR_INVALID, "capacities must be positive (max_caption_len >= 2)");
    LRP_HIP_CHECK(hipSetDevice(cfg->device));
    lrp_handle* h = new lrp_handle();
    h->cfg = *cfg;
    if (cfg->encoder != LRP_ENC_VGG && cfg->encoder != LRP_ENC_RESNET) {
      delete h;
      return fail(LRP_ERR_UNSUPPORTED, "unknown encoder kind %d", cfg->encoder);
    }
    h->resnet = cfg->encoder == LRP_ENC_RESNET;
    int rc = h->resnet ? h->rn.init(*cfg, &h->ws_bytes) : h->enc.init(*cfg, &h->ws_bytes);
    if (rc == LRP_OK) rc = h->dec.init(*cfg, &h->ws_bytes);
    if (rc == LRP_OK) rc = h->idx_dev.alloc((size_t)cfg->max_tokens * 2 * sizeof(int), &h->ws_bytes);
    if (rc == LRP_OK) rc = h->rfeat_tmp.alloc((size_t)cfg->max_tokens * cfg->L * cfg->D * sizeof(float), &h->ws_bytes);
    if (rc == LRP_OK && hipHostMalloc(reinterpret_cast<void**>(&h->idx_pinned), (size_t)cfg->max_tokens * 2 * sizeof(int)) != hipSuccess)
      rc = fail(LRP_ERR_NOMEM, "hipHostMalloc for index staging failed");
    if (rc != LRP_OK) {
      delete h;
      return rc;
    }
    *out = h;
    return LRP_OK;
  });
}

int lrp_destroy(lrp_handle* h) {
  return guarded([&]() -> int {
    if (!h) return LRP_OK;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    delete h;
    return LRP_OK;
  });
}

int64_t lrp_workspace_bytes(const lrp_handle* h) { return h ? h->ws_bytes : 0; }

// One body for both weight setters: name routing, shape checks, then the array is copied into HBM (`kind`: from the
// caller's host or device memory) and every operand copy is built there by the device packers (cnn_kernels.h pack_*_dev,
// resnet_encoder.h pack_unit_dev, Decoder::repack_device).  Everything is enqueued on `st`; nothing waits for it.
static int set_weight(lrp_handle* h, const char* name, const float* data, hipMemcpyKind kind, int32_t ndim, const int64_t* shape,
                      hipStream_t st) {
  if (!name || !data || !shape || ndim < 1 || ndim > 4) return fail(LRP_ERR_INVALID, "bad lrp_set_weight arguments");
  LRP_TRY(h->trainer.drop_early_forward(nullptr));   // an lrp_train_forward of the old weights is stale
  const std::string nm(name);
  if (h->resnet) {
    if (h->dec.known_weight(nm)) return h->dec.set_weight(nm, data, kind, ndim, shape, &h->ws_bytes, st);
    const int rc = h->rn.set_weight(nm, data, kind, ndim, shape, &h->ws_bytes, st);
    if (rc != 1) return rc;                         // 1 = not an encoder weight
    return fail(LRP_ERR_INVALID, "unknown weight '%s'", name);
  }
  if (nm.size() > 2 && (nm.compare(nm.size() - 2, 2, "_W") == 0 || nm.compare(nm.size() - 2, 2, "_b") == 0)) {
    const int li = h->enc.find_layer(nm.substr(0, nm.size() - 2));
    if (li >= 0) {
      const ConvLayer& L = h->enc.layers[li];
      if (nm.back() == 'W') {
        if (ndim != 4 || shape[0] != 3 || shape[1] != 3 || shape[2] != L.cin || shape[3] != L.cout)
          return fail(LRP_ERR_INVALID, "%s: expected HWIO (3,3,%d,%d)", name, L.cin, L.cout);
        return h->enc.set_conv_weight_dev(li, data, kind, &h->ws_bytes, st);
      }
      if (ndim != 1 || shape[0] != L.cout) return fail(LRP_ERR_INVALID, "%s: expected (%d,)", name, L.cout);
      return h->enc.set_conv_bias_dev(li, data, kind, &h->ws_bytes, st);
    }
  }
  return h->dec.set_weight(nm, data, kind, ndim, shape, &h->ws_bytes, st);
}

// Synchronous: on return the caller's array has been read (it may be reused or freed) and errors of the copy have surfaced.
int lrp_set_weight(lrp_handle* h, const char* name, const float* data_host, int32_t ndim, const int64_t* shape) {
  return with_handle(h, [&]() -> int {
    const int rc = set_weight(h, name, data_host, hipMemcpyHostToDevice, ndim, shape, nullptr);
    if (rc != LRP_OK) {
      (void)hipStreamSynchronize(nullptr);               // (a copy out of the caller's array may already be in flight)
      return rc;
    }
    LRP_HIP_CHECK(hipStreamSynchronize(nullptr));
    return LRP_OK;
  });
}

// The multi-GPU start-up path: the bundle arrives in HBM over RCCL/xGMI and stays there.  No device-to-host copy, no
// stream synchronisation.
int lrp_set_weight_dev(lrp_handle* h, const char* name, const float* data_dev, int32_t ndim, const int64_t* shape,
                       void* stream) {
  return with_handle(h, [&]() -> int {
    return set_weight(h, name, data_dev, hipMemcpyDeviceToDevice, ndim, shape, S(stream));
  });
}

int lrp_encode_images(lrp_handle* h, const float* images_dev, int32_t B, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !images_dev) return fail(LRP_ERR_INVALID, "null argument");
    LRP_TRY(h->trainer.drop_early_forward(S(stream)));   // it read the features this call overwrites
    LRP_TRY(h->resnet ? h->rn.encode(images_dev, B, S(stream)) : h->enc.encode(images_dev, B, S(stream)));
    return h->dec.on_new_features(B);
  });
}

int lrp_set_features(lrp_handle* h, const float* features_dev, int32_t B, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !features_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (B < 1 || B > h->cfg.max_images) return fail(LRP_ERR_INVALID, "B=%d outside [1,%d]", B, h->cfg.max_images);
    LRP_TRY(h->trainer.drop_early_forward(S(stream)));
    LRP_HIP_CHECK(hipMemcpyAsync(h->feat(), features_dev, (size_t)B * h->cfg.L * h->cfg.D * sizeof(float),
                                 hipMemcpyDeviceToDevice, S(stream)));
    h->encoded() = B;
    h->features_only() = true;
    return h->dec.on_new_features(B);
  });
}

int lrp_get_features(lrp_handle* h, float* features_dev, int32_t B, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !features_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (B < 1 || B > h->encoded()) return fail(LRP_ERR_STATE, "only %d images are cached", h->encoded());
    LRP_HIP_CHECK(hipMemcpyAsync(features_dev, h->feat(), (size_t)B * h->cfg.L * h->cfg.D * sizeof(float),
                                 hipMemcpyDeviceToDevice, S(stream)));
    return LRP_OK;
  });
}

int lrp_decoder_forward(lrp_handle* h, const int32_t* captions_host, const int32_t* lengths_host, int32_t B, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !captions_host || !lengths_host) return fail(LRP_ERR_INVALID, "null argument");
    if (B < 1 || B > h->encoded()) return fail(LRP_ERR_STATE, "B=%d but %d images have features cached", B, h->encoded());
    return h->dec.forward(h->feat(), captions_host, lengths_host, B, S(stream));
  });
}

int lrp_decoder_gen_begin(lrp_handle* h, int32_t B, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    if (B < 1 || B > h->encoded()) return fail(LRP_ERR_STATE, "B=%d but %d images have features cached", B, h->encoded());
    return h->dec.gen_begin(h->feat(), B, S(stream));
  });
}

int lrp_decoder_gen_step(lrp_handle* h, int32_t B, const int32_t* parent_host, const int32_t* word_host, int32_t step,
                         double* logits_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !logits_dev || (step > 0 && (!parent_host || !word_host))) return fail(LRP_ERR_INVALID, "null argument");
    return h->dec.gen_step(B, parent_host, word_host, step, logits_dev, S(stream));
  });
}

int lrp_decoder_beam_search(lrp_handle* h, int32_t n_images, int32_t k, int32_t steps, int32_t eos, int32_t* captions_dev,
                            int32_t* lengths_dev, double* logp_dev, int32_t* n_complete_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !captions_dev || !lengths_dev || !logp_dev || !n_complete_dev) return fail(LRP_ERR_INVALID, "null argument");
    return h->dec.beam_search(n_images, k, steps, eos, captions_dev, lengths_dev, logp_dev, n_complete_dev, S(stream));
  });
}

int lrp_read_state(lrp_handle* h, const char* name, void* out_dev, size_t out_bytes, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !name || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    return h->dec.read_state(name, out_dev, out_bytes, S(stream));
  });
}

// stage (img_idx | t) into device memory; validates ranges against the cached captions
static int stage_indices(lrp_handle* h, int n, const int32_t* img_idx, const int32_t* t, bool need_t, hipStream_t st) {
  if (n < 1 || n > h->cfg.max_tokens) return fail(LRP_ERR_INVALID, "n=%d outside [1,%d]", n, h->cfg.max_tokens);
  // the pinned staging buffer may still feed the previous call's copy: wait for THAT copy only (no stream sync —
  // the stream usually holds the decoder replay at this point, and draining it would leave the GPU idle while the
  // host enqueues the explain launches)
  if (!h->ev_idx) LRP_HIP_CHECK(hipEventCreateWithFlags(&h->ev_idx, hipEventDisableTiming));
  else LRP_HIP_CHECK(hipEventSynchronize(h->ev_idx));
  for (int i = 0; i < n; ++i) {
    if (img_idx[i] < 0 || img_idx[i] >= h->encoded())
      return fail(LRP_ERR_INVALID, "img_idx[%d]=%d outside the %d cached images", i, img_idx[i], h->encoded());
    h->idx_pinned[i] = img_idx[i];
    if (need_t) {
      LRP_TRY(h->dec.check_token(img_idx[i], t[i]));
      h->idx_pinned[n + i] = t[i];
    }
  }
  LRP_HIP_CHECK(hipMemcpyAsync(h->idx_dev.p, h->idx_pinned, (size_t)n * (need_t ? 2 : 1) * sizeof(int), hipMemcpyHostToDevice, st));
  LRP_HIP_CHECK(hipEventRecord(h->ev_idx, st));
  return LRP_OK;
}

int lrp_decoder_explain(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const int32_t* t_host, int32_t variant,
                        float* R_feat_dev, float* att_dev, double* r_words_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !img_idx_host || !t_host || !R_feat_dev) return fail(LRP_ERR_INVALID, "null argument");
    LRP_TRY(stage_indices(h, n, img_idx_host, t_host, true, S(stream)));
    return h->dec.explain(n, h->idx_dev.as<int>(), h->idx_dev.as<int>() + n, img_idx_host, t_host, variant,
                          h->feat(), R_feat_dev, att_dev, r_words_dev, S(stream));
  });
}

int lrp_cnn_explain(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const float* R_feat_dev, float* R_img_dev,
                    void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !img_idx_host || !R_feat_dev || !R_img_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (h->encoded() < 1 || h->features_only()) return fail(LRP_ERR_STATE, "lrp_encode_images must run before lrp_cnn_explain");
    LRP_TRY(stage_indices(h, n, img_idx_host, nullptr, false, S(stream)));
    if (h->resnet) return h->rn.explain(n, h->idx_dev.as<int>(), R_feat_dev, R_img_dev, S(stream));
    h->enc.row2img_host = h->idx_pinned;
    return h->enc.explain(n, h->idx_dev.as<int>(), R_feat_dev, R_img_dev, S(stream));
  });
}

// ---- layer trace (Encoder::explain_traced) ----
int lrp_set_layer_trace(lrp_handle* h, int32_t on) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    if (on != 0 && on != 1) return fail(LRP_ERR_INVALID, "on must be 0 or 1");
    if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "the layer trace is built for the VGG-style (conv-list) encoders only");
    if ((on != 0) == h->enc.tr.on) return LRP_OK;
    LRP_TRY(h->trainer.drop_early_forward(nullptr));      // (it ran on the caches this drops)
    return h->enc.set_layer_trace(on != 0, &h->ws_bytes);
  });
}

int32_t lrp_trace_tensor_count(lrp_handle* h) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "the layer trace is built for the VGG-style (conv-list) encoders only");
    return (int)h->enc.trace_tensors().size();
  });
}

int lrp_trace_tensor_info(lrp_handle* h, int32_t index, int32_t n, uint64_t keep_mask, int32_t* nid, int32_t* H, int32_t* W, int32_t* C,
                          int64_t* offset, int64_t* keep_floats) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "the layer trace is built for the VGG-style (conv-list) encoders only");
    const std::vector<TraceTensor> tt = h->enc.trace_tensors();
    if (index < 0 || index >= (int)tt.size()) return fail(LRP_ERR_INVALID, "tensor %d outside [0,%d)", index, (int)tt.size());
    if (n < 1 || n > h->enc.max_tokens) return fail(LRP_ERR_INVALID, "n=%d outside [1,%d]", n, h->enc.max_tokens);
    if (tt.size() < 64 && (keep_mask >> tt.size()) != 0) return fail(LRP_ERR_INVALID, "keep_mask names tensors beyond the %d traced", (int)tt.size());
    std::vector<int64_t> off;
    const int64_t total = h->enc.trace_keep_layout(n, keep_mask, off);
    const TraceTensor& t = tt[(size_t)index];
    if (nid) *nid = t.nid;
    if (H) *H = t.H;
    if (W) *W = t.W;
    if (C) *C = t.C;
    if (offset) *offset = off[(size_t)index];
    if (keep_floats) *keep_floats = total;
    return LRP_OK;
  });
}

int lrp_cnn_explain_traced(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const float* R_feat_dev, float* R_img_dev,
                           double* stats_dev, uint64_t keep_mask, float* keep_dev, int64_t keep_floats, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !img_idx_host || !R_feat_dev || !R_img_dev || !stats_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (h->resnet)
      return fail(LRP_ERR_UNSUPPORTED, "the layer trace is built for the VGG-style (conv-list) encoders only (a ResNet's reversed graph has "
                                       "some 350 nodes of six kinds, and its walk fuses several of them)");
    // (checked before any staging: nothing runs on a refusal)
    LRP_TRY(h->enc.trace_check(n));
    const size_t nt = h->enc.trace_tensors().size();
    if (nt < 64 && (keep_mask >> nt) != 0) return fail(LRP_ERR_INVALID, "keep_mask names tensors beyond the %d traced", (int)nt);
    std::vector<int64_t> off;
    const int64_t need = h->enc.trace_keep_layout(n, keep_dev ? keep_mask : 0, off);
    if (keep_dev && keep_floats < need)
      return fail(LRP_ERR_INVALID, "the keep buffer holds %lld floats, the selected tensors need %lld (lrp_trace_tensor_info)",
                  (long long)keep_floats, (long long)need);
    LRP_TRY(stage_indices(h, n, img_idx_host, nullptr, false, S(stream)));
    return h->enc.explain_traced(n, h->idx_dev.as<int>(), R_feat_dev, R_img_dev, stats_dev, keep_dev, off, S(stream));
  });
}

int lrp_op_tensor_stats(const float* x_dev, int32_t rows, int64_t per_row, double* stats_dev, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !stats_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (rows < 1 || per_row < 1) return fail(LRP_ERR_INVALID, "rows and per_row must be positive");
    return Encoder::tensor_stats(x_dev, rows, (size_t)per_row, stats_dev, S(stream));
  });
}

int lrp_explain_tokens(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const int32_t* t_host, int32_t variant,
                       float* R_img_dev, float* R_feat_dev, float* att_dev, double* r_words_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !img_idx_host || !t_host || !R_img_dev) return fail(LRP_ERR_INVALID, "null argument");
    LRP_TRY(stage_indices(h, n, img_idx_host, t_host, true, S(stream)));
    float* rf = R_feat_dev ? R_feat_dev : h->rfeat_tmp.as<float>();
    LRP_TRY(h->dec.explain(n, h->idx_dev.as<int>(), h->idx_dev.as<int>() + n, img_idx_host, t_host, variant,
                           h->feat(), rf, att_dev, r_words_dev, S(stream)));
    if (h->resnet) return h->rn.explain(n, h->idx_dev.as<int>(), rf, R_img_dev, S(stream));
    h->enc.row2img_host = h->idx_pinned;
    return h->enc.explain(n, h->idx_dev.as<int>(), rf, R_img_dev, S(stream));
  });
}

int lrp_decoder_gradient(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const int32_t* t_host, float* d_feat_dev,
                         double* r_words_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !img_idx_host || !t_host || !d_feat_dev) return fail(LRP_ERR_INVALID, "null argument");
    // (checked before any staging, allocation or launch: nothing runs)
    if (h->cfg.decoder == LRP_DEC_ADAPTIVE && h->cfg.E != h->cfg.H)
      return fail(LRP_ERR_UNSUPPORTED, "the adaptive gradient baseline needs E == H (E=%d, H=%d): the reference's class cannot run there "
                                       "(explainers.py:798 sizes d_xt E + H wide, :823 stores a 2E-wide row into it and raises), so "
                                       "no reference defines the result",
                  h->cfg.E, h->cfg.H);
    LRP_TRY(stage_indices(h, n, img_idx_host, t_host, true, S(stream)));
    int t_max = 0;
    for (int i = 0; i < n; ++i) t_max = t_host[i] > t_max ? t_host[i] : t_max;
    return h->dec.gradient(n, h->idx_dev.as<int>(), h->idx_dev.as<int>() + n, t_max, d_feat_dev, r_words_dev, &h->ws_bytes,
                           S(stream));
  });
}

int lrp_cnn_walk(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const float* head_dev, float* out_dev, int32_t walk,
                 void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !img_idx_host || !head_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (walk < LRP_WALK_LRP || walk > LRP_WALK_PATTERN_ATTRIBUTION) return fail(LRP_ERR_INVALID, "unknown walk %d", walk);
    if (walk == LRP_WALK_PATTERNNET || walk == LRP_WALK_PATTERN_ATTRIBUTION) {   // (as DeepLIFT: its own checks, nothing runs on a refusal)
      if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "the pattern walks are built for the VGG-style (conv-list) encoders only");
      LRP_TRY(h->enc.pattern_walk_check(n));
      LRP_TRY(stage_indices(h, n, img_idx_host, nullptr, false, S(stream)));
      return h->enc.explain_pattern(n, h->idx_dev.as<int>(), head_dev, out_dev, walk == LRP_WALK_PATTERN_ATTRIBUTION, S(stream));
    }
    if (walk == LRP_WALK_DEEPLIFT) {                     // (its own checks, in its own order: mode before state; nothing runs on a refusal)
      if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "the DeepLIFT walk is built for the VGG-style (conv-list) encoders only");
      LRP_TRY(h->enc.dl_check(n));
      LRP_TRY(stage_indices(h, n, img_idx_host, nullptr, false, S(stream)));
      return h->enc.explain_deeplift(n, h->idx_dev.as<int>(), head_dev, out_dev, S(stream));
    }
    if (h->encoded() < 1 || h->features_only()) return fail(LRP_ERR_STATE, "lrp_encode_images must run before lrp_cnn_walk");
    // (checked before any staging: nothing runs; Deconvnet reads no ReLU decision and runs in every mode)
    if (h->resnet && walk != LRP_WALK_LRP && walk != LRP_WALK_DECONVNET && h->rn.prec != PREC_FP32)
      return fail(LRP_ERR_UNSUPPORTED, "gradient walks on a ResNet encoder run in LRP_PREC_FP32 only: set it with lrp_set_precision "
                                       "and call lrp_encode_images again");
    LRP_TRY(stage_indices(h, n, img_idx_host, nullptr, false, S(stream)));
    if (h->resnet) return h->rn.explain(n, h->idx_dev.as<int>(), head_dev, out_dev, S(stream), walk);
    h->enc.row2img_host = h->idx_pinned;
    return h->enc.explain(n, h->idx_dev.as<int>(), head_dev, out_dev, S(stream), walk);
  });
}

// ---- PatternNet / PatternAttribution (Encoder::pattern_*) ----
static int pattern_handle(lrp_handle* h) {
  if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "patterns are built for the VGG-style (conv-list) encoders only (the reference refuses BatchNorm and Add too)");
  return LRP_OK;
}
static int pattern_conv(lrp_handle* h, int32_t conv) {
  LRP_TRY(pattern_handle(h));
  if (conv < 0 || conv >= (int)h->enc.layers.size()) return fail(LRP_ERR_INVALID, "conv %d outside [0,%d)", conv, (int)h->enc.layers.size());
  return LRP_OK;
}

int lrp_pattern_fit_begin(lrp_handle* h, int32_t type) {
  return with_handle(h, [&]() -> int {
    LRP_TRY(pattern_handle(h));
    static_assert(LRP_PATTERN_LINEAR == lrp::PAT_LINEAR && LRP_PATTERN_RELU_POSITIVE == lrp::PAT_RELU_POSITIVE &&
                  LRP_PATTERN_RELU_NEGATIVE == lrp::PAT_RELU_NEGATIVE, "lrp_hip.h LRP_PATTERN_*");
    if (type < LRP_PATTERN_LINEAR || type > LRP_PATTERN_RELU_NEGATIVE) return fail(LRP_ERR_INVALID, "unknown pattern type %d", type);
    LRP_TRY(h->enc.pattern_mode_check());
    LRP_TRY(h->trainer.drop_early_forward(nullptr));      // (it ran on the caches this drops)
    return h->enc.pattern_fit_begin(type, &h->ws_bytes);
  });
}

int lrp_pattern_fit_batch(lrp_handle* h, void* stream) {
  return with_handle(h, [&]() -> int {
    LRP_TRY(pattern_handle(h));
    return h->enc.pattern_fit_batch(S(stream));
  });
}

int lrp_pattern_fit_end(lrp_handle* h, void* stream) {
  return with_handle(h, [&]() -> int {
    LRP_TRY(pattern_handle(h));
    return h->enc.pattern_fit_end(S(stream));
  });
}

int lrp_pattern_stats(lrp_handle* h, int32_t conv, double* sums_dev, int64_t n_doubles, void* stream) {
  return with_handle(h, [&]() -> int {
    LRP_TRY(pattern_conv(h, conv));
    if (!sums_dev) return fail(LRP_ERR_INVALID, "null argument");
    const ConvLayer& L = h->enc.layers[(size_t)conv];
    const DevBuf& sums = h->enc.pat.layer[(size_t)conv].sums;
    const size_t doubles = PatternState::sum_doubles(L.cin, L.cout);
    if (n_doubles != (int64_t)doubles)
      return fail(LRP_ERR_INVALID, "conv %d: the sums are %lld doubles (2 x 9 cin cout + 2 cout + 1), %lld given", conv,
                  (long long)doubles, (long long)n_doubles);
    if (!sums.p) return fail(LRP_ERR_STATE, "no fit has run: lrp_pattern_fit_begin allocates the sums");
    LRP_HIP_CHECK(hipMemcpyAsync(sums_dev, sums.p, doubles * sizeof(double), hipMemcpyDeviceToDevice, S(stream)));
    return LRP_OK;
  });
}

int lrp_set_patterns(lrp_handle* h, int32_t conv, const float* A_hwio_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    LRP_TRY(pattern_conv(h, conv));
    if (!A_hwio_dev) return fail(LRP_ERR_INVALID, "null argument");
    return h->enc.pattern_set(conv, A_hwio_dev, S(stream));
  });
}

int lrp_get_patterns(lrp_handle* h, int32_t conv, float* A_hwio_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    LRP_TRY(pattern_conv(h, conv));
    if (!A_hwio_dev) return fail(LRP_ERR_INVALID, "null argument");
    const ConvLayer& L = h->enc.layers[(size_t)conv];
    const PatternState::Layer& pl = h->enc.pat.layer[(size_t)conv];
    if (!pl.have) return fail(LRP_ERR_STATE, "conv %d has no pattern: fit them (lrp_pattern_fit_*) or set them (lrp_set_patterns)", conv);
    LRP_HIP_CHECK(hipMemcpyAsync(A_hwio_dev, pl.A.p, (size_t)9 * L.cin * L.cout * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    return LRP_OK;
  });
}

int lrp_set_pattern_projection(lrp_handle* h, int32_t on) {
  return with_handle(h, [&]() -> int {
    LRP_TRY(pattern_handle(h));
    if (on != 0 && on != 1) return fail(LRP_ERR_INVALID, "on must be 0 or 1");
    h->enc.pat.project = on != 0;
    return LRP_OK;
  });
}

int lrp_set_precision(lrp_handle* h, int32_t mode) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    if (mode != LRP_PREC_FP32 && mode != LRP_PREC_BF16X3 && mode != LRP_PREC_BF16X3_FAST && mode != LRP_PREC_F16X2)
      return fail(LRP_ERR_INVALID, "unknown precision mode %d", mode);
    const int km = mode == LRP_PREC_FP32 ? PREC_FP32 : PREC_BF16X3;
    const bool fast = mode == LRP_PREC_BF16X3_FAST, f16 = mode == LRP_PREC_F16X2;
    // The encode caches belong to the arithmetic they were computed in (the gates' denominators Z+ follow the walk's
    // products; the fp32 mode takes another forward altogether): a mode change drops them, so that an explain call
    // without a new lrp_encode_images returns LRP_ERR_STATE instead of walking with gates of the other arithmetic.
    if (h->enc.prec != km || h->enc.fwd_fast != fast || h->enc.walk_f16 != f16) {
      LRP_TRY(h->trainer.drop_early_forward(nullptr));
      h->enc.encoded = 0;
      h->rn.encoded = 0;
      h->enc.dl.ref_stale = true;                        // (the DeepLIFT reference's activations go with the caches)
    }
    h->enc.prec = km;
    h->enc.fwd_fast = fast;
    h->enc.walk_f16 = f16;                            // (forward, decoder and the ResNet encoder stay as in LRP_PREC_BF16X3)
    h->rn.prec = km;
    return LRP_OK;
  });
}

// The rule of a VGG handle, from either entry: `t` is validated, one record per conv.  Alpha-beta with the bias and beta == 0 on every
// conv is the default walk, which is the empty table.
static int set_vgg_table(lrp_handle* h, std::vector<ConvRule> t) {
  Encoder& e = h->enc;
  bool is_default = true;
  for (const ConvRule& r : t)
    if (r.kind != LRP_RULE_ALPHA_BETA || !r.bias || r.beta > 0.f) is_default = false;
  if (is_default) t.clear();
  bool same = t.size() == e.rules.table.size();          // the same rule again changes nothing
  for (size_t i = 0; same && i < t.size(); ++i) {
    const ConvRule &a = e.rules.table[i], &b = t[i];
    if (a.kind != b.kind || a.bias != b.bias || a.alpha != b.alpha || a.eps != b.eps || a.low != b.low || a.high != b.high) same = false;
  }
  if (same) return LRP_OK;
  LRP_TRY(h->trainer.drop_early_forward(nullptr));
  if (t.empty()) {
    e.clear_table();
    return LRP_OK;
  }
  LRP_TRY(e.set_table(t, &h->ws_bytes));
  if (h->trainer.ready) {
    // the fine-tune step owns the weights (the layers' own HWIO copies are gone after its first update): the table's matrices
    // come from its master buffer, here, once per rule change
    for (size_t li = 0; li < e.layers.size(); ++li)
      LRP_TRY(e.pack_table_layer((int)li, h->trainer.master.as<float>() + h->trainer.params[2 * li].off, nullptr));
    LRP_HIP_CHECK(hipStreamSynchronize(nullptr));
  }
  return LRP_OK;
}

int lrp_set_cnn_rule(lrp_handle* h, float alpha, float beta) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    // relevance_based/utils.py:72-129 (the caller's binding infers an omitted parameter and words the errors as the reference does)
    if (!(alpha >= 1.f)) return fail(LRP_ERR_INVALID, "alpha should be >= 1 (alpha=%g)", (double)alpha);
    if (!(beta >= 0.f)) return fail(LRP_ERR_INVALID, "beta should be >= 0 (beta=%g)", (double)beta);
    // alpha - beta == 1 holds for the caller's numbers, which reach this entry rounded to float each (1.3f - 0.3f = 1 - 2^-24): the
    // pair is accepted when it is 1 to that rounding (half an ulp of each operand), and the walk's beta is then alpha - 1, which
    // is exact in float for alpha in [1, 2] and the nearest float beyond — so the relevance the rule conserves is conserved
    if (!(fabs((double)alpha - (double)beta - 1.0) <= 6e-8 * ((double)alpha + (double)beta)))
      return fail(LRP_ERR_INVALID, "alpha - beta should be 1 (alpha=%g, beta=%g)", (double)alpha, (double)beta);
    beta = alpha - 1.f;
    if (h->resnet) return h->rn.set_rule(alpha, beta);    // (refuses beta > 0 on widths that are no multiples of 8)
    ConvRule r;                                          // the one rule is a uniform table (with the bias, as RR:274-322 has it)
    r.alpha = alpha; r.beta = beta;
    return set_vgg_table(h, std::vector<ConvRule>(h->enc.layers.size(), r));
  });
}

// One record of either rule entry, value-checked into `o`.  i: the conv the record is for, 0 = the input layer — flat, w-square and
// bounded are refused above it
static int check_conv_rule(const lrp_conv_rule& r, int i, ConvRule& o) {
  if (r.kind < LRP_RULE_ALPHA_BETA || r.kind > LRP_RULE_BOUNDED) return fail(LRP_ERR_INVALID, "conv %d: unknown rule kind %d", i, r.kind);
  o.kind = r.kind;
  if (o.input_only() && i > 0)
    return fail(LRP_ERR_INVALID, "conv %d: flat, w-square and bounded are input-layer rules (above it they need relevance at dead units)", i);
  o.bias = 0;
  if (r.kind == LRP_RULE_ALPHA_BETA || r.kind == LRP_RULE_EPSILON) {
    if (r.bias != 0 && r.bias != 1) return fail(LRP_ERR_INVALID, "conv %d: bias must be 0 or 1", i);
    o.bias = r.bias;
  }
  if (r.kind == LRP_RULE_ALPHA_BETA) {               // lrp_set_cnn_rule's check
    if (!(r.alpha >= 1.f)) return fail(LRP_ERR_INVALID, "conv %d: alpha should be >= 1 (alpha=%g)", i, (double)r.alpha);
    if (!(r.beta >= 0.f)) return fail(LRP_ERR_INVALID, "conv %d: beta should be >= 0 (beta=%g)", i, (double)r.beta);
    if (!(fabs((double)r.alpha - (double)r.beta - 1.0) <= 6e-8 * ((double)r.alpha + (double)r.beta)))
      return fail(LRP_ERR_INVALID, "conv %d: alpha - beta should be 1 (alpha=%g, beta=%g)", i, (double)r.alpha, (double)r.beta);
    o.alpha = r.alpha; o.beta = r.alpha - 1.f;
  } else if (r.kind == LRP_RULE_EPSILON) {
    if (!(r.eps >= 0.f) || !(r.eps < 3.0e38f)) return fail(LRP_ERR_INVALID, "conv %d: epsilon should be >= 0 (eps=%g)", i, (double)r.eps);
    o.eps = r.eps;
  } else if (r.kind == LRP_RULE_BOUNDED) {
    if (!(r.low < r.high) || !(fabsf(r.low) < 3.0e38f) || !(fabsf(r.high) < 3.0e38f))
      return fail(LRP_ERR_INVALID, "bounded rule: low < high (low=%g, high=%g)", (double)r.low, (double)r.high);
    o.low = r.low; o.high = r.high;
  }
  return LRP_OK;
}

int lrp_set_cnn_rules(lrp_handle* h, const lrp_conv_rule* rules, int32_t n_rules) {
  return with_handle(h, [&]() -> int {
    if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "the ResNet encoder's walk has no rule per conv: lrp_set_resnet_rules takes a rule pair");
    if (!rules || n_rules != (int)h->enc.layers.size())
      return fail(LRP_ERR_INVALID, "one rule per conv: %d given, %d convs", rules ? n_rules : 0, (int)h->enc.layers.size());
    std::vector<ConvRule> t((size_t)n_rules);
    for (int i = 0; i < n_rules; ++i) LRP_TRY(check_conv_rule(rules[i], i, t[(size_t)i]));
    if (t[0].input_only() && n_rules < 2) return fail(LRP_ERR_UNSUPPORTED, "an input-layer rule needs a conv above the image layer");
    return set_vgg_table(h, std::move(t));
  });
}

int lrp_set_deeplift_reference(lrp_handle* h, const float* ref_host, float ref_scalar, int32_t mode) {
  return with_handle(h, [&]() -> int {
    if (mode < 0 || mode > 2) return fail(LRP_ERR_INVALID, "DeepLIFT mode %d: 0 = off, 1 = approximate_gradient=False, 2 = True", mode);
    if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "the DeepLIFT walk is built for the VGG-style (conv-list) encoders only");
    const int was = h->enc.encoded;
    LRP_TRY(h->enc.set_deeplift_reference(ref_host, ref_scalar, mode, &h->ws_bytes));
    if (was && !h->enc.encoded) LRP_TRY(h->trainer.drop_early_forward(nullptr));   // (a change dropped the caches it ran on)
    return LRP_OK;
  });
}

int lrp_set_resnet_rules(lrp_handle* h, const lrp_conv_rule* stem, const lrp_conv_rule* units) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    if (!h->resnet) return fail(LRP_ERR_UNSUPPORTED, "a VGG-style handle takes a rule per conv: lrp_set_cnn_rules");
    if (!stem || !units) return fail(LRP_ERR_INVALID, "lrp_set_resnet_rules: two records, the stem's and the other convs'");
    ConvRule cs, cu;
    LRP_TRY(check_conv_rule(*stem, 0, cs));
    LRP_TRY(check_conv_rule(*units, 1, cu));
    auto rec = [](const ConvRule& c) {
      ResNetEncoder::Rule r;
      r.kind = c.kind; r.bias = c.bias; r.alpha = c.alpha; r.beta = c.beta; r.eps = c.eps; r.low = c.low; r.high = c.high;
      return r;
    };
    return h->rn.set_rules(rec(cs), rec(cu));                      // (refuses beta > 0 on widths that are no multiples of 8)
  });
}

int lrp_set_fast_layers(lrp_handle* h, int64_t mask) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    const int nl = (int)h->enc.layers.size();
    if (mask < -1 || (mask >= 0 && nl < 63 && (mask >> nl) != 0)) return fail(LRP_ERR_INVALID, "mask 0x%llx names layers beyond the %d convs", (unsigned long long)mask, nl);
    if (mask >= 0 && (mask & 1)) return fail(LRP_ERR_INVALID, "layer 0 (the image layer) has no two-term form");
    if (h->enc.t2_mask_user != mask && h->enc.walk_f16) {   // the denominators follow the walk: the caches belong to the old choice
      LRP_TRY(h->trainer.drop_early_forward(nullptr));
      h->enc.encoded = 0;
    }
    h->enc.t2_mask_user = mask;
    return LRP_OK;
  });
}

int lrp_profile_enable(lrp_handle* h, int32_t on) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    h->enc.prof.on = on != 0;
    h->rn.prof.on = on != 0;
    return LRP_OK;
  });
}

int lrp_profile_query(lrp_handle* h, int64_t* n_launches, double* total_ms, double* total_flop) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    return (h->resnet ? h->rn.prof : h->enc.prof).query(n_launches, total_ms, total_flop);
  });
}

int lrp_profile_records(lrp_handle* h, int32_t cap, double* ms_out, double* flop_out, int32_t* n_out) {
  return with_handle(h, [&]() -> int {
    if (!h || !ms_out || !flop_out || !n_out || cap < 0) return fail(LRP_ERR_INVALID, "bad lrp_profile_records arguments");
    return (h->resnet ? h->rn.prof : h->enc.prof).records(cap, ms_out, flop_out, n_out);
  });
}

// Operator entries: the caller's HWIO array (taps, Cin, Cout) goes to HBM as it is (`raw`, uploaded once) and is packed there
// by the packer the handles use (cnn_kernels.h pack_conv_dev_kernel): forward [Cout rows][taps * CinP], or — bwd — the
// transposed conv's [Cin rows][taps * CoutP] with flipped taps; zero padded.
static int op_pack_weight(const float* w_host, int taps, int Cin, int Cout, int bwd, DevBuf& raw, DevBuf& pk, hipStream_t st) {
  if (!raw.p) {
    LRP_TRY(raw.alloc((size_t)taps * Cin * Cout * sizeof(float), nullptr));
    LRP_HIP_CHECK(hipMemcpy(raw.p, w_host, raw.bytes, hipMemcpyHostToDevice));
  }
  const int rows = conv_npad(bwd ? Cin : Cout), CP = conv_cinp(bwd ? Cout : Cin);
  const size_t tot = (size_t)rows * taps * CP;
  LRP_TRY(pk.alloc(tot * sizeof(float), nullptr));
  hipLaunchKernelGGL(pack_conv_dev_kernel, dim3(stream_grid(tot)), dim3(256), 0, st, raw.as<float>(), pk.as<float>(), bwd, Cin, Cout, CP,
                     rows, 0, 0, taps);
  LRP_HIP_CHECK(hipGetLastError());
  return LRP_OK;
}

int lrp_op_conv(const float* in_dev, const float* w_hwio_host, const float* bias_host, const float* aux_dev, float* out_dev,
                int32_t NB, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t taps, int32_t mode, void* stream) {
  return guarded([&]() -> int {
    if (!in_dev || !w_hwio_host || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (taps != 1 && taps != 9) return fail(LRP_ERR_INVALID, "taps must be 1 or 9");
    if (Cin % 4 != 0) return fail(LRP_ERR_UNSUPPORTED, "Cin must be a multiple of 4");
    const bool split = (mode & LRP_CONV_SPLIT_BF16) != 0;   // same op on the split-bf16 MFMA path (fp32 in, fp32 out)
    const bool wreg = (mode & LRP_CONV_WREG) != 0;          // ... with the fragment-major weight copy of the 128 x 128 weights-in-registers loop
    mode &= ~(LRP_CONV_SPLIT_BF16 | LRP_CONV_WREG);
    if (mode < 0 || mode > 3) return fail(LRP_ERR_INVALID, "mode must be 0..3");
    if (split && mode == 0) return fail(LRP_ERR_UNSUPPORTED, "the split-bf16 path has no relu epilogue (modes 1..3)");
    const bool bwd = mode >= 2;
    // forward: in has Cin channels, out Cout.  backward: in has Cout channels (S), out Cin (relevance of the input)
    const int inC = bwd ? Cout : Cin, outC = bwd ? Cin : Cout;
    static const int epi_of_mode[4] = {EPI_BIAS_RELU, EPI_BIAS, EPI_MUL, EPI_MUL_UP2};
    // (the bit asks for what the default switches would make: LRP_CONV_BREG4=0 then puts the same copy on the pipelined kernel)
    if (wreg && !(split && (conv_frag_forms(epi_of_mode[mode], PREC_BF16X3, 7, outC, inC, taps, Switches()) & (1u << FORM_BREG4))))
      return fail(LRP_ERR_UNSUPPORTED, "LRP_CONV_WREG needs LRP_CONV_SPLIT_BF16, mode 2, 9 taps and Cin %% 128 == 0");
    if (inC % 4 != 0) return fail(LRP_ERR_UNSUPPORTED, "input channels must be a multiple of 4");
    if (split && ((inC & 7) || (bwd && (outC & 7)))) return fail(LRP_ERR_UNSUPPORTED, "split-bf16 path: channels must be multiples of 8");
    const int Np = conv_npad(outC), K = taps * conv_cinp(inC);
    hipStream_t st = S(stream);
    DevBuf wraw, wdev, wsplit, bdev, insplit, wfrag;
    LRP_TRY(op_pack_weight(w_hwio_host, taps, Cin, Cout, bwd, wraw, wdev, st));
    if (split) {
      const size_t nw8 = (size_t)Np * K / 8;
      LRP_TRY(wsplit.alloc(wdev.bytes, nullptr));
      hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(nw8)), dim3(256), 0, st, wdev.as<float>(), wsplit.as<float>(), nw8);
      // weights-in-registers variants of the backward convs
      if (wreg || conv_frag_forms(epi_of_mode[mode], PREC_BF16X3, 7, outC, inC, taps)) {
        LRP_TRY(wfrag.alloc((size_t)Np * K * sizeof(float), nullptr));
        hipLaunchKernelGGL(pack_frag_dev_kernel, dim3(stream_grid((size_t)conv_cinp(inC) / 32 * 9 * 8 * Np)), dim3(256), 0, st,
                           wsplit.as<float>(), wfrag.as<float>(), conv_cinp(inC), Np);
      }
      const size_t n8 = (size_t)NB * H * W * inC / 8;
      LRP_TRY(insplit.alloc(n8 * 32, nullptr));
      hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(n8)), dim3(256), 0, st, in_dev, insplit.as<float>(), n8);
      LRP_HIP_CHECK(hipGetLastError());
      in_dev = insplit.as<float>();
    }
    ConvArgs ca{};
    ca.out_plain = 1;
    ca.wpk_frag = wfrag.as<float>();
    ca.in = in_dev; ca.wpk = split ? wsplit.as<float>() : wdev.as<float>(); ca.NB = NB; ca.H = H; ca.W = W; ca.Cin = inC; ca.CinP = conv_cinp(inC);
    ca.N = outC; ca.taps = taps; ca.out = out_dev; ca.aux = aux_dev;
    if (!bwd) {
      if (!bias_host) return fail(LRP_ERR_INVALID, "bias required for forward modes");
      LRP_TRY(bdev.alloc((size_t)Cout * sizeof(float), nullptr));
      LRP_HIP_CHECK(hipMemcpy(bdev.p, bias_host, (size_t)Cout * sizeof(float), hipMemcpyHostToDevice));
      ca.bias = bdev.as<float>();
    } else if (!aux_dev) {
      return fail(LRP_ERR_INVALID, "aux (gate) required for backward modes");
    }
    if (split && !wreg && ca.wpk_frag) {                   // without the bit a 128 x 128 launch keeps the pipelined kernel
      const ConvPlan p = conv_plan(conv_ask(epi_of_mode[mode], PREC_BF16X3, 7, false, ca));
      if (p.ok && p.form == FORM_BREG4) ca.wpk_frag = nullptr;
    }
    LRP_HIP_CHECK(conv_launch(epi_of_mode[mode], ca, st, split ? PREC_BF16X3 : PREC_FP32));
    LRP_HIP_CHECK(hipStreamSynchronize(st));             // weights are freed on return
    return LRP_OK;
  });
}

int lrp_op_conv_rule(const float* s0_dev, const float* s1_dev, const float* w_hwio_host, int32_t chains_in, int32_t gates_out, float p0,
                     float q0, float p1, float q1, const float* g0_dev, const float* g1_dev, float* out0_dev, float* out1_dev, int32_t NB,
                     int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pool, int32_t split, void* stream) {
  return guarded([&]() -> int {
    if ((chains_in != 1 && chains_in != 2) || (gates_out != 1 && gates_out != 2)) return fail(LRP_ERR_INVALID, "chains_in and gates_out are 1 or 2");
    if (!s0_dev || !w_hwio_host || !g0_dev || !out0_dev || (chains_in == 2 && !s1_dev) || (gates_out == 2 && (!g1_dev || !out1_dev)))
      return fail(LRP_ERR_INVALID, "null argument");
    if (NB < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return fail(LRP_ERR_INVALID, "NB, H, W, Cin, Cout must be >= 1");
    const int g = split ? 7 : 3;
    if ((Cin & g) || (Cout & g)) return fail(LRP_ERR_UNSUPPORTED, "channels must be multiples of %d", g + 1);
    {
      ConvAsk q;                                         // the launch below, as conv_launch will ask for it
      q.epi = pool ? EPI_MUL_UP2 : EPI_MUL; q.prec = split ? PREC_BF16X3 : PREC_FP32;
      q.NB = NB; q.H = H; q.W = W; q.N = Cin; q.Cin = chains_in * Cout; q.taps = 9; q.dual_mul = gates_out == 2;
      if (!conv_plan(q).ok)
        return fail(LRP_ERR_UNSUPPORTED, "no launch reads %d chain(s) of %d channels into %d gate(s) of %d", chains_in, Cout, gates_out, Cin);
    }
    const int64_t up = pool ? 4 : 1, lim = (int64_t)1 << 31;
    if ((int64_t)NB * H * W * 2 * Cout >= lim || (int64_t)9 * Cin * Cout >= lim || (int64_t)NB * H * W * up * Cin * gates_out >= lim)
      return fail(LRP_ERR_UNSUPPORTED, "operator entry: tensor too large");
    hipStream_t st = S(stream);
    const int CPk = conv_cinp(chains_in * Cout), Np = conv_npad(Cin);
    DevBuf wraw, wk, wks, sj;
    LRP_TRY(wraw.alloc((size_t)9 * Cin * Cout * sizeof(float), nullptr));
    LRP_HIP_CHECK(hipMemcpy(wraw.p, w_hwio_host, wraw.bytes, hipMemcpyHostToDevice));
    const size_t nb = (size_t)Np * 9 * CPk;
    LRP_TRY(wk.alloc(nb * sizeof(float), nullptr));
    LRP_HIP_CHECK(hipMemsetAsync(wk.p, 0, wk.bytes, st));
    hipLaunchKernelGGL(pack_conv_rule_dev_kernel, dim3(stream_grid((size_t)Cin * 9 * CPk)), dim3(256), 0, st, wraw.as<float>(), wk.as<float>(), 1,
                       Cin, Cout, CPk, Cin, chains_in, p0, q0, p1, q1);
    const size_t pixels = (size_t)NB * H * W;
    const float* in = s0_dev;
    if (chains_in == 2 || split) LRP_TRY(sj.alloc(pixels * chains_in * Cout * sizeof(float), nullptr));
    if (split) {
      LRP_TRY(wks.alloc(nb * sizeof(float), nullptr));
      hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(nb / 8)), dim3(256), 0, st, wk.as<float>(), wks.as<float>(), nb / 8);
      if (chains_in == 2)
        hipLaunchKernelGGL(chain_join_kernel<true>, dim3(stream_grid(pixels * (Cout / 8))), dim3(256), 0, st, s0_dev, s1_dev, (const float*)nullptr,
                           (const float*)nullptr, (const int*)nullptr, sj.as<float>(), pixels, 1, Cout);
      else
        hipLaunchKernelGGL(split_copy_kernel, dim3(stream_grid(pixels * Cout / 8)), dim3(256), 0, st, s0_dev, sj.as<float>(), pixels * Cout / 8);
      in = sj.as<float>();
    } else if (chains_in == 2) {
      hipLaunchKernelGGL(chain_join_kernel<false>, dim3(stream_grid(pixels * (Cout / 4))), dim3(256), 0, st, s0_dev, s1_dev, (const float*)nullptr,
                         (const float*)nullptr, (const int*)nullptr, sj.as<float>(), pixels, 1, Cout);
      in = sj.as<float>();
    }
    LRP_HIP_CHECK(hipGetLastError());
    ConvArgs ca{};
    ca.in = in; ca.wpk = split ? wks.as<float>() : wk.as<float>();
    ca.NB = NB; ca.H = H; ca.W = W; ca.Cin = chains_in * Cout; ca.CinP = CPk; ca.N = Cin; ca.taps = 9;
    ca.aux = g0_dev; ca.out = out0_dev; ca.out_plain = 1;
    if (gates_out == 2) { ca.aux_b = g1_dev; ca.out_b = out1_dev; ca.ostride = Cin; }
    LRP_HIP_CHECK(conv_launch(pool ? EPI_MUL_UP2 : EPI_MUL, ca, st, split ? PREC_BF16X3 : PREC_FP32));
    LRP_HIP_CHECK(hipStreamSynchronize(st));             // the operand copies are freed on return
    return LRP_OK;
  });
}

// the two-chain launch of alpha-beta with beta > 0: both chains in, both gates out, [alpha w+ ; -beta w-]
int lrp_op_conv_ab(const float* sp_dev, const float* sn_dev, const float* w_hwio_host, float alpha, float beta, const float* gp_dev,
                   const float* gn_dev, float* outp_dev, float* outn_dev, int32_t NB, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                   int32_t pool, int32_t split, void* stream) {
  return lrp_op_conv_rule(sp_dev, sn_dev, w_hwio_host, 2, 2, alpha, 0.f, 0.f, -beta, gp_dev, gn_dev, outp_dev, outn_dev, NB, H, W, Cin, Cout, pool,
                          split, stream);
}

// One fused conv + ReLU layer of the DeepLIFT walk (Encoder::explain_deeplift) as an operator.  Image and reference go through the
// forward as ONE batch of NB + 1 (the same launch: where they agree on a receptive field Y and Yr are the same bits); a three-channel
// input takes the image layer's forms (im2col GEMM forward, tap-expanded GEMM + stencil backward) as layer 0 of a handle does.
int lrp_op_deeplift_conv(const float* x_dev, const float* xr_dev, const float* a_dev, const float* w_hwio_host, const float* bias_host,
                         float* out_dev, int32_t NB, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pool, int32_t mode, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !xr_dev || !a_dev || !w_hwio_host || !bias_host || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (mode != 1 && mode != 2) return fail(LRP_ERR_INVALID, "DeepLIFT mode %d: 1 = approximate_gradient=False, 2 = True", mode);
    if (NB < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return fail(LRP_ERR_INVALID, "NB, H, W, Cin, Cout must be >= 1");
    const bool img = Cin == 3;
    if ((Cout & 3) || (!img && (Cin & 3))) return fail(LRP_ERR_UNSUPPORTED, "Cout must be a multiple of 4, Cin 3 or a multiple of 4");
    if (pool && ((H & 1) || (W & 1))) return fail(LRP_ERR_UNSUPPORTED, "odd resolution before a 2x2 pool");
    const bool two = mode == 2;
    const int rows = two ? 2 * NB : NB, NF = NB + 1;
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)rows * H * W * std::max(Cout, img ? IMG_T_COLS : Cin) >= lim || (int64_t)NF * H * W * std::max(2 * Cout, 64) >= lim ||
        (int64_t)9 * Cin * Cout >= lim)
      return fail(LRP_ERR_UNSUPPORTED, "operator entry: tensor too large");
    hipStream_t st = S(stream);
    const size_t px = (size_t)H * W, xin = px * Cin, act = px * Cout;
    DevBuf xa, y, z, a1, wraw, wf, wb, wb2, bdev, gm, pooled, D, Sb, Cb, Tb, r2i;
    // ---- the launches, each asked of conv_plan before the first one runs ----
    ConvArgs cf{}, cb{};
    int epi_f, epi_b;
    if (img) {
      cf.NB = NF * H * W; cf.H = 1; cf.W = 1; cf.Cin = 64; cf.CinP = 64; cf.taps = 1; cf.N = 2 * Cout; cf.split = Cout;
      epi_f = EPI_FWD_DUAL;
      cb.NB = rows; cb.H = H; cb.W = W; cb.Cin = Cout; cb.CinP = conv_cinp(Cout); cb.taps = 1; cb.N = IMG_T_COLS;
      if (Encoder::img_fused()) { cb.img_mode = 1; epi_b = EPI_IMG_STENCIL; }
      else { cb.NB = rows * H * W; cb.H = 1; cb.W = 1; epi_b = EPI_STORE; }
    } else {
      cf.NB = NF; cf.H = H; cf.W = W; cf.Cin = Cin; cf.CinP = conv_cinp(Cin); cf.taps = 9; cf.N = Cout;
      epi_f = EPI_BIAS_RELU;
      cb.NB = rows; cb.H = H; cb.W = W; cb.Cin = Cout; cb.CinP = conv_cinp(Cout); cb.taps = 9; cb.N = Cin; cb.gate_none = 1;
      epi_b = EPI_MUL;
    }
    if (!conv_plan(conv_ask(epi_f, PREC_FP32, 7, false, cf)).ok || !conv_plan(conv_ask(epi_b, PREC_FP32, 7, false, cb)).ok)
      return fail(LRP_ERR_UNSUPPORTED, "no exact-fp32 launch for a %d -> %d layer at %d x %d", Cin, Cout, H, W);
    // ---- forward of [x ; xr] ----
    LRP_TRY(xa.alloc((size_t)NF * xin * sizeof(float), nullptr));
    LRP_HIP_CHECK(hipMemcpyAsync(xa.p, x_dev, (size_t)NB * xin * sizeof(float), hipMemcpyDeviceToDevice, st));
    LRP_HIP_CHECK(hipMemcpyAsync(xa.as<float>() + (size_t)NB * xin, xr_dev, xin * sizeof(float), hipMemcpyDeviceToDevice, st));
    LRP_TRY(y.alloc((size_t)NF * act * sizeof(float), nullptr));
    LRP_TRY(bdev.alloc((size_t)Cout * sizeof(float), nullptr));
    LRP_HIP_CHECK(hipMemcpy(bdev.p, bias_host, (size_t)Cout * sizeof(float), hipMemcpyHostToDevice));
    if (img) {
      const size_t nf = (size_t)conv_npad(2 * Cout) * 64, nb = (size_t)conv_npad(IMG_T_COLS) * conv_cinp(Cout);
      LRP_TRY(wraw.alloc((size_t)27 * Cout * sizeof(float), nullptr));
      LRP_HIP_CHECK(hipMemcpy(wraw.p, w_hwio_host, wraw.bytes, hipMemcpyHostToDevice));
      LRP_TRY(wf.alloc(nf * sizeof(float), nullptr)); LRP_TRY(wb2.alloc(nb * sizeof(float), nullptr)); LRP_TRY(wb.alloc(nb * sizeof(float), nullptr));
      LRP_HIP_CHECK(hipMemsetAsync(wf.p, 0, wf.bytes, st)); LRP_HIP_CHECK(hipMemsetAsync(wb2.p, 0, wb2.bytes, st));
      LRP_HIP_CHECK(hipMemsetAsync(wb.p, 0, wb.bytes, st));
      hipLaunchKernelGGL(pack_image_layer_dev_kernel, dim3((27 * Cout + 255) / 256), dim3(256), 0, st, wraw.as<float>(), wf.as<float>(), wb2.as<float>(),
                         wb.as<float>(), Cout, conv_cinp(Cout));
      LRP_TRY(a1.alloc((size_t)NF * px * 64 * sizeof(float), nullptr));
      LRP_TRY(z.alloc((size_t)NF * act * sizeof(float), nullptr));
      hipLaunchKernelGGL(im2col_image_kernel, dim3((unsigned)(((size_t)NF * px * 8 + 255) / 256)), dim3(256), 0, st, xa.as<float>(), a1.as<float>(), NF, H, W);
      LRP_HIP_CHECK(hipGetLastError());
      cf.in = a1.as<float>(); cf.out2 = z.as<float>();
    } else {
      LRP_TRY(op_pack_weight(w_hwio_host, 9, Cin, Cout, 0, wraw, wf, st));
      LRP_TRY(op_pack_weight(w_hwio_host, 9, Cin, Cout, 1, wraw, wb, st));
      cf.in = xa.as<float>();
    }
    cf.wpk = wf.as<float>(); cf.bias = bdev.as<float>(); cf.out = y.as<float>();
    LRP_HIP_CHECK(conv_launch(epi_f, cf, st, PREC_FP32));
    // ---- the gate D of the layer: the mask of the images' forward (through the pool: its first arg-max), safe(Y - Yr) under it ----
    const float* yr = y.as<float>() + (size_t)NB * act;
    LRP_TRY(D.alloc((size_t)NB * act * sizeof(float), nullptr));
    if (pool) {
      LRP_TRY(gm.alloc((size_t)NB * act * sizeof(float), nullptr));
      LRP_TRY(pooled.alloc((size_t)NB * act / 4 * sizeof(float), nullptr));
      hipLaunchKernelGGL(pool_gate_kernel, dim3(stream_grid((size_t)NB * act / 16)), dim3(256), 0, st, y.as<float>(), y.as<float>(), pooled.as<float>(),
                         gm.as<float>(), NB, H, W, Cout);             // (z = a: the gate is 1 at a live arg-max, 0 elsewhere)
    }
    hipLaunchKernelGGL(dl_gate_kernel, dim3(stream_grid((size_t)NB * act / 4)), dim3(256), 0, st, pool ? (const float*)nullptr : y.as<float>(),
                       pool ? gm.as<float>() : (const float*)nullptr, pool ? pooled.as<float>() : (const float*)nullptr, yr, D.as<float>(), NB, H, W, Cout);
    LRP_HIP_CHECK(hipGetLastError());
    // ---- the chains [a / D ; a M] (routed through the pool), the transposed conv over both, the select ----
    LRP_TRY(Sb.alloc((size_t)rows * act * sizeof(float), nullptr));
    const int Ha = pool ? H / 2 : H, Wa = pool ? W / 2 : W;
    LRP_TRY(Encoder::dl_combine(two, pool != 0, a_dev, nullptr, nullptr, D.as<float>(), nullptr, Sb.as<float>(), NB, Ha, Wa, Cout, st));
    LRP_TRY(Cb.alloc((size_t)rows * px * (img ? 4 : Cin) * sizeof(float), nullptr));
    cb.in = Sb.as<float>(); cb.wpk = wb.as<float>(); cb.out = Cb.as<float>();
    if (img) {
      std::vector<int> idx((size_t)rows);
      for (int i = 0; i < rows; ++i) idx[(size_t)i] = i % NB;
      LRP_TRY(r2i.alloc((size_t)rows * sizeof(int), nullptr));
      LRP_HIP_CHECK(hipMemcpy(r2i.p, idx.data(), (size_t)rows * sizeof(int), hipMemcpyHostToDevice));
      cb.row2img = r2i.as<int>(); cb.ximg = xa.as<float>();
      if (epi_b == EPI_STORE) {
        LRP_TRY(Tb.alloc((size_t)rows * px * IMG_T_COLS * sizeof(float), nullptr));
        cb.out = Tb.as<float>();
      }
    }
    LRP_HIP_CHECK(conv_launch(epi_b, cb, st, PREC_FP32));
    if (img && epi_b == EPI_STORE) {
      hipLaunchKernelGGL(img_stencil_kernel, dim3(stream_grid((size_t)rows * px)), dim3(256), 0, st, Tb.as<float>(), xa.as<float>(), r2i.as<int>(),
                         Cb.as<float>(), rows, H, W, 1, 0.f, 0.f);
      LRP_HIP_CHECK(hipGetLastError());
    }
    LRP_TRY(Encoder::dl_final(two, Cb.as<float>(), x_dev, xr_dev, nullptr, out_dev, NB, xin, st));
    LRP_HIP_CHECK(hipStreamSynchronize(st));             // the operand copies are freed on return
    return LRP_OK;
  });
}

int lrp_op_conv_pool_sparse(const float* sc_dev, const unsigned char* pos_dev, const float* w_hwio_host, const float* gate_dev,
                            float* out_dev, int32_t NB, int32_t Hp, int32_t Wp, int32_t Cin, int32_t Cout, int32_t reps, void* stream) {
  return guarded([&]() -> int {
    if (!sc_dev || !pos_dev || !w_hwio_host || !gate_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (NB < 1 || Hp < 1 || Wp < 1 || (reps & 255) < 1) return fail(LRP_ERR_INVALID, "NB, Hp, Wp, reps must be >= 1");
    if (!conv_sparse_supports(Cin, Cout, Hp, Wp))
      return fail(LRP_ERR_UNSUPPORTED, "the sparse consumer needs Cin %% 256 == 0 (output columns) and Cout %% 16 == 0");
    hipStream_t st = S(stream);
    DevBuf wraw, wb, wsp, pairs;
    LRP_TRY(op_pack_weight(w_hwio_host, 9, Cin, Cout, 1, wraw, wb, st));
    LRP_TRY(wsp.alloc(conv_sparse_weight_floats(Cin, Cout) * sizeof(float), nullptr));
    LRP_HIP_CHECK(conv_sparse_pack(wb.as<float>(), wsp.as<float>(), Cin, Cout, st));
    const size_t n8 = (size_t)NB * Hp * Wp * Cout / 8;
    LRP_TRY(pairs.alloc(n8 * 32, nullptr));
    LRP_HIP_CHECK(conv_sparse_pairs(sc_dev, pairs.as<float>(), NB, Hp, Wp, Cout, st));
    DevBuf idxp;
    LRP_TRY(idxp.alloc(conv_sparse_index_words(NB, Hp, Wp, Cout) * sizeof(unsigned), nullptr));
    LRP_HIP_CHECK(conv_sparse_index(pos_dev, idxp.as<unsigned>(), NB, Hp, Wp, Cout, st));
    SparseArgs sa{};
    sa.sc = pairs.as<float>(); sa.idxp = idxp.as<unsigned>(); sa.wsp = wsp.as<float>(); sa.gate = gate_dev; sa.out = out_dev;
    sa.NB = NB; sa.Hp = Hp; sa.Wp = Wp; sa.C = Cout; sa.N = Cin; sa.out_plain = 1;
    sa.diag = reps >> 8;                                   // (measurement variants, profiles/sparse_ab.py: bit 0 leaves the results meaningless; bits 1 / 2 force a tile form)
    reps &= 255;
    for (int r = 0; r < reps; ++r) LRP_HIP_CHECK(conv_sparse_launch(sa, st));
    LRP_HIP_CHECK(hipStreamSynchronize(st));               // the operand copies are freed on return
    return LRP_OK;
  });
}

int lrp_op_epsilon_dense(const float* x_dev, const float* W_host, const float* R_dev, float* out_dev, int32_t N,
                         int32_t Din, int32_t Dout, float epsilon, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !W_host || !R_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (N < 1 || (Din & 3) || (Dout & 3) || !(epsilon > 0.f)) return fail(LRP_ERR_INVALID, "need N>=1, Din%%4==0, Dout%%4==0, epsilon>0");
    hipStream_t st = S(stream);
    // Z = x.W  (1-tap GEMM, B operand packed [Dout][Din]);  C = S.W^T  (packed [Din][Dout])
    const int K = conv_cinp(Din), Kb = conv_cinp(Dout);
    DevBuf wraw, wf, wb, Z, Sb;
    LRP_TRY(op_pack_weight(W_host, 1, Din, Dout, 0, wraw, wf, st));
    LRP_TRY(op_pack_weight(W_host, 1, Din, Dout, 1, wraw, wb, st));
    LRP_TRY(Z.alloc((size_t)N * Dout * sizeof(float), nullptr));
    LRP_TRY(Sb.alloc((size_t)N * Dout * sizeof(float), nullptr));
    ConvArgs cz{};
    cz.in = x_dev; cz.wpk = wf.as<float>(); cz.NB = N; cz.H = 1; cz.W = 1; cz.Cin = Din; cz.CinP = K; cz.N = Dout; cz.taps = 1;
    cz.out = Z.as<float>();
    LRP_HIP_CHECK(conv_launch(EPI_STORE, cz, st));
    const size_t ne = (size_t)N * Dout;
    hipLaunchKernelGGL(eps_divide_kernel, dim3(stream_grid(ne)), dim3(256), 0, st, R_dev, Z.as<float>(), Sb.as<float>(), epsilon, ne);
    LRP_HIP_CHECK(hipGetLastError());
    ConvArgs cb{};
    cb.in = Sb.as<float>(); cb.wpk = wb.as<float>(); cb.NB = N; cb.H = 1; cb.W = 1; cb.Cin = Dout; cb.CinP = Kb; cb.N = Din;
    cb.taps = 1; cb.aux = x_dev; cb.out = out_dev;
    LRP_HIP_CHECK(conv_launch(EPI_MUL, cb, st));                       // R_in = x * (S . W^T)
    LRP_HIP_CHECK(hipStreamSynchronize(st));
    return LRP_OK;
  });
}

int lrp_op_batchnorm_lrp(const float* x_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev,
                         const float* var_dev, float bn_eps, const float* R_dev, float* out_dev, int64_t n, int32_t C,
                         void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !gamma_dev || !beta_dev || !mean_dev || !var_dev || !R_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || C < 1 || n % C) return fail(LRP_ERR_INVALID, "n must be a positive multiple of C");
    hipLaunchKernelGGL(bn_lrp_kernel, dim3(stream_grid((size_t)n)), dim3(256), 0, S(stream), x_dev, gamma_dev, beta_dev,
                       mean_dev, var_dev, bn_eps, R_dev, out_dev, (size_t)n, C);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_add_lrp(const float* a_dev, const float* b_dev, const float* R_dev, float* Ra_dev, float* Rb_dev, int64_t n,
                   void* stream) {
  return guarded([&]() -> int {
    if (!a_dev || !b_dev || !R_dev || !Ra_dev || !Rb_dev || n < 1) return fail(LRP_ERR_INVALID, "bad argument");
    hipLaunchKernelGGL(add_lrp_kernel, dim3(stream_grid((size_t)n)), dim3(256), 0, S(stream), a_dev, b_dev, R_dev, Ra_dev,
                       Rb_dev, (size_t)n);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_avgpool_lrp(const float* x_dev, const float* R_dev, float* out_dev, int32_t NB, int32_t H, int32_t W, int32_t C,
                       int32_t k, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !R_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (NB < 1 || k < 1 || H < k || W < k || (H % k) || (W % k)) return fail(LRP_ERR_UNSUPPORTED, "need H, W multiples of the pool size");
    if (C < 4 || (C & 3)) return fail(LRP_ERR_UNSUPPORTED, "C must be a multiple of 4");
    const size_t total = (size_t)NB * (H / k) * (W / k) * (C / 4);
    hipLaunchKernelGGL(avgpool_lrp_kernel, dim3(stream_grid(total)), dim3(256), 0, S(stream), x_dev, R_dev, out_dev, NB, H, W, C, k);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_heatmap_render(const float* R_img_dev, const float* lut_dev, float* rgb_dev, int32_t n, int32_t npix, int32_t C,
                       float gamma, void* stream) {
  return guarded([&]() -> int {
    if (!R_img_dev || !lut_dev || !rgb_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || npix < 1 || C < 1 || !(gamma > 0.f)) return fail(LRP_ERR_INVALID, "n, npix, C, gamma must be positive");
    hipLaunchKernelGGL(heatmap_render_kernel, dim3(n), dim3(256), 0, S(stream), R_img_dev, lut_dev, rgb_dev, npix, C, gamma);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_preprocess_images(const uint8_t* rgb_dev, float* out_dev, int32_t NB, int32_t H0, int32_t W0, int32_t H, int32_t W,
                          void* stream) {
  return guarded([&]() -> int {
    if (!rgb_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (NB < 1 || H0 < 1 || W0 < 1 || H < 1 || W < 1) return fail(LRP_ERR_INVALID, "sizes must be positive");
    hipLaunchKernelGGL(preprocess_caffe_kernel, dim3(stream_grid((size_t)NB * H * W)), dim3(256), 0, S(stream), rgb_dev, out_dev,
                       NB, H0, W0, H, W);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

// ---- operator-level entries of the fine-tune step's products (unit tests of train_gemm.h at real layer sizes)
int lrp_op_sgemm(const float* A_dev, const float* B_dev, float* C_dev, int32_t M, int32_t N, int64_t K, int64_t lda, int64_t ldb,
                 int64_t ldc, int32_t transA, int32_t transB, int32_t accumulate, float* ws_dev, int64_t ws_floats, void* stream) {
  return guarded([&]() -> int {
    if (!A_dev || !B_dev || !C_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (M < 1 || N < 1 || K < 1 || (transA && transB)) return fail(LRP_ERR_INVALID, "bad sgemm shape / transposes");
    SgemmArgs a{};
    a.A = A_dev; a.B = B_dev; a.C = C_dev; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
    a.transA = transA != 0; a.transB = transB != 0; a.accumulate = accumulate != 0;
    LRP_HIP_CHECK(sgemm(a, ws_dev, ws_dev ? (size_t)ws_floats : 0, S(stream)));
    return LRP_OK;
  });
}

static int op_conv_wgrad(bool bf16, const float* x_dev, const float* dz_dev, float* dw_hwio_dev, float* db_dev, int32_t NB, int32_t H,
                         int32_t W, int32_t Cin, int32_t Cout, float* ws_dev, int64_t ws_floats, void* stream) {
  if (!x_dev || !dz_dev || !dw_hwio_dev || !ws_dev) return fail(LRP_ERR_INVALID, "null argument");
  if (NB < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return fail(LRP_ERR_INVALID, "sizes must be positive");
  if (ws_floats < (int64_t)2 * 9 * Cin * Cout) return fail(LRP_ERR_INVALID, "workspace smaller than 2 x 9 x Cin x Cout floats");
  SgemmArgs a{};
  a.A = x_dev; a.lda = Cin; a.B = dz_dev; a.ldb = Cout; a.C = dw_hwio_dev; a.ldc = Cout;
  a.M = Cin; a.N = Cout; a.K = (long)NB * H * W; a.transA = 1;
  a.gather = 1; a.gH = H; a.gW = W; a.taps = 9; a.tapC = (long)Cin * Cout;
  if (bf16) LRP_HIP_CHECK(wgrad_bf16(a, ws_dev, (size_t)ws_floats, S(stream)));
  else LRP_HIP_CHECK(sgemm(a, ws_dev, (size_t)ws_floats, S(stream)));
  if (db_dev) LRP_HIP_CHECK(colsum(dz_dev, Cout, (long)NB * H * W, Cout, db_dev, 0, ws_dev, (size_t)ws_floats, S(stream)));
  return LRP_OK;
}

int lrp_op_conv_wgrad(const float* x_dev, const float* dz_dev, float* dw_hwio_dev, float* db_dev, int32_t NB, int32_t H, int32_t W,
                      int32_t Cin, int32_t Cout, float* ws_dev, int64_t ws_floats, void* stream) {
  return guarded([&]() -> int {
    return op_conv_wgrad(false, x_dev, dz_dev, dw_hwio_dev, db_dev, NB, H, W, Cin, Cout, ws_dev, ws_floats, stream);
  });
}

int lrp_op_conv_wgrad_bf16(const float* x_dev, const float* dz_dev, float* dw_hwio_dev, float* db_dev, int32_t NB, int32_t H,
                           int32_t W, int32_t Cin, int32_t Cout, float* ws_dev, int64_t ws_floats, void* stream) {
  return guarded([&]() -> int {
    return op_conv_wgrad(true, x_dev, dz_dev, dw_hwio_dev, db_dev, NB, H, W, Cin, Cout, ws_dev, ws_floats, stream);
  });
}

// ---- fine-tune step, trainer.h
int lrp_train_begin(lrp_handle* h, float lr, float clipvalue, float beta1, float beta2, float eps) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null handle");
    if (h->resnet) return fail(LRP_ERR_UNSUPPORTED, "the fine-tune step is built for the VGG encoder");
    if (!(lr > 0.f) || clipvalue < 0.f || !(eps > 0.f)) return fail(LRP_ERR_INVALID, "lr, eps must be positive, clipvalue >= 0");
    LRP_HIP_CHECK(hipSetDevice(h->cfg.device));
    return h->trainer.begin(h->enc, h->dec, h->cfg, lr, clipvalue, beta1, beta2, eps, &h->ws_bytes);
  });
}

int lrp_train_set_precision(lrp_handle* h, int32_t mode) {
  return with_handle(h, [&]() -> int {
    if (mode != LRP_TRAIN_FP32 && mode != LRP_TRAIN_BF16) return fail(LRP_ERR_INVALID, "unknown training precision %d", mode);
    h->trainer.train_prec = mode;
    return LRP_OK;
  });
}

int64_t lrp_train_flat_size(const lrp_handle* h) { return h && h->trainer.ready ? (int64_t)h->trainer.n_total : 0; }
int32_t lrp_train_num_params(const lrp_handle* h) { return h && h->trainer.ready ? (int32_t)h->trainer.params.size() : 0; }

int lrp_train_param_info(const lrp_handle* h, int32_t i, const char** name, int64_t* offset, int64_t* size) {
  return with_handle(h, [&]() -> int {
    if (!h || !h->trainer.ready) return fail(LRP_ERR_STATE, "lrp_train_begin must run first");
    if (i < 0 || i >= (int32_t)h->trainer.params.size()) return fail(LRP_ERR_INVALID, "parameter index %d out of range", i);
    const TrainParam& p = h->trainer.params[i];
    if (name) *name = p.name.c_str();
    if (offset) *offset = (int64_t)p.off;
    if (size) *size = (int64_t)p.n;
    return LRP_OK;
  });
}

int lrp_train_step(lrp_handle* h, int32_t B, int32_t T, const int32_t* cap_in_dev, const int32_t* y_idx_dev,
                   const float* lrp_weight_dev, const float* mask_image_features_dev, const float* mask_global_dev,
                   const float* mask_output_dev, const float* mask_lstm_in_dev, const float* mask_lstm_rec_dev,
                   const float* mask_logits_dev, float* grads_dev, float* losses_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !cap_in_dev || !y_idx_dev || !lrp_weight_dev || !grads_dev) return fail(LRP_ERR_INVALID, "null argument");
    Trainer::StepIn in{};
    in.feat = h->feat(); in.B = B; in.T = T; in.cap_in = cap_in_dev; in.y_idx = y_idx_dev; in.lrp_weight = lrp_weight_dev;
    in.m_if = mask_image_features_dev; in.m_glob = mask_global_dev; in.m_out = mask_output_dev; in.m_lin = mask_lstm_in_dev;
    in.m_lrec = mask_lstm_rec_dev; in.m_logits = mask_logits_dev; in.grads = grads_dev; in.losses_dev = losses_dev; in.st = S(stream);
    return h->trainer.step(h->enc, in, &h->ws_bytes);
  });
}

int lrp_train_forward(lrp_handle* h, int32_t B, int32_t T, const int32_t* cap_in_dev, const float* mask_image_features_dev,
                      const float* mask_global_dev, const float* mask_output_dev, const float* mask_lstm_in_dev,
                      const float* mask_lstm_rec_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !cap_in_dev) return fail(LRP_ERR_INVALID, "null argument");
    Trainer::StepIn in{};
    in.feat = h->feat(); in.B = B; in.T = T; in.cap_in = cap_in_dev;
    in.m_if = mask_image_features_dev; in.m_glob = mask_global_dev; in.m_out = mask_output_dev; in.m_lin = mask_lstm_in_dev;
    in.m_lrec = mask_lstm_rec_dev; in.st = S(stream);
    return h->trainer.forward(h->enc, in, &h->ws_bytes);
  });
}

int lrp_train_drop_forward(lrp_handle* h, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h) return fail(LRP_ERR_INVALID, "null argument");
    return h->trainer.drop_early_forward(S(stream));
  });
}

int lrp_train_apply(lrp_handle* h, const float* grads_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !grads_dev) return fail(LRP_ERR_INVALID, "null argument");
    return h->trainer.apply(h->enc, h->dec, grads_dev, S(stream));
  });
}

int lrp_train_get_master(lrp_handle* h, float* flat_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !flat_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (!h->trainer.ready) return fail(LRP_ERR_STATE, "lrp_train_begin must run first");
    LRP_HIP_CHECK(hipMemcpyAsync(flat_dev, h->trainer.master.p, h->trainer.n_total * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    return LRP_OK;
  });
}

int lrp_heatmap_scores(const float* R_img_dev, double* scores_dev, int32_t n, int32_t npix, int32_t C, int32_t mode,
                       void* stream) {
  return guarded([&]() -> int {
    if (!R_img_dev || !scores_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || npix < 1 || C < 1) return fail(LRP_ERR_INVALID, "n, npix, C must be positive");
    if (mode < 0 || mode > 2) return fail(LRP_ERR_UNSUPPORTED, "the lrp inference mode is not available");
    hipLaunchKernelGGL(heatmap_score_kernel, dim3(n), dim3(256), 0, S(stream), R_img_dev, scores_dev, npix, C, mode);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_log_softmax_topk(const double* logits_dev, int32_t rows, int32_t V, int32_t k, int32_t* ids_dev, double* logp_dev,
                            void* stream) {
  return guarded([&]() -> int {
    if (!logits_dev || !ids_dev || !logp_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (rows < 1 || V < 1 || k < 1 || k > V || k > TOPK_MAX) return fail(LRP_ERR_INVALID, "need rows >= 1 and 1 <= k <= min(V, %d)", TOPK_MAX);
    hipLaunchKernelGGL(log_softmax_topk_kernel, dim3(rows), dim3(256), 0, S(stream), logits_dev, V, k, ids_dev, logp_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

// ---- the beam bookkeeping as stand-alone operators on caller-owned buffers (csrc/beam_kernels.h)
static int beam_op_args(int n_images, int k, int max_len) {
  if (n_images < 1 || max_len < 1 || k < 1 || k > BEAM_K_MAX)
    return fail(LRP_ERR_INVALID, "need n_images >= 1, max_len >= 1 and 1 <= k <= %d", BEAM_K_MAX);
  if ((int64_t)n_images * k * k > INT32_MAX || (int64_t)n_images * k * (max_len + 1) > INT32_MAX)
    return fail(LRP_ERR_INVALID, "n_images x k x k and n_images x k x (max_len + 1) must fit 31 bits");
  return LRP_OK;
}

int64_t lrp_op_beam_state_bytes(int32_t n_images, int32_t k, int32_t max_len) {
  return guarded([&]() -> int { return beam_op_args(n_images, k, max_len); }) == LRP_OK
             ? (int64_t)beam_state_bytes(n_images, k, max_len)
             : (int64_t)LRP_ERR_INVALID;
}

int lrp_op_beam_select(void* state_dev, const int32_t* ids_dev, const double* logp_dev, int32_t n_images, int32_t k, int32_t max_len,
                       int32_t step, int32_t eos, int32_t* parent_dev, int32_t* word_dev, void* stream) {
  return guarded([&]() -> int {
    if (!state_dev || !ids_dev || !logp_dev || !parent_dev || !word_dev) return fail(LRP_ERR_INVALID, "null argument");
    LRP_TRY(beam_op_args(n_images, k, max_len));
    if (step < 0 || step >= max_len) return fail(LRP_ERR_RANGE, "step %d outside [0,%d)", step, max_len);
    hipLaunchKernelGGL(beam_select_kernel, dim3(n_images), dim3(BEAM_THREADS), 0, S(stream), state_dev, ids_dev, logp_dev, k, max_len,
                       step, eos, parent_dev, word_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_beam_finish(const void* state_dev, int32_t n_images, int32_t k, int32_t max_len, int32_t steps, int32_t eos,
                       int32_t* captions_dev, int32_t* lengths_dev, double* logp_dev, int32_t* n_complete_dev, void* stream) {
  return guarded([&]() -> int {
    if (!state_dev || !captions_dev || !lengths_dev || !logp_dev || !n_complete_dev) return fail(LRP_ERR_INVALID, "null argument");
    LRP_TRY(beam_op_args(n_images, k, max_len));
    if (steps < 1 || steps > max_len) return fail(LRP_ERR_RANGE, "steps=%d outside [1,%d]", steps, max_len);
    hipLaunchKernelGGL(beam_finish_kernel, dim3(n_images), dim3(64), 0, S(stream), state_dev, k, max_len, steps, eos, captions_dev,
                       lengths_dev, logp_dev, n_complete_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

// ---- bounding-box correctness evaluation (csrc/eval_kernels.h; evaluate_bbox.py)
static int eval_expand_matrix(int g, int up, double sigma, double* M) {
  // pyramid_expand(A, upscale, sigma) = G R A R^T G^T: R (S x g) the bilinear resize of skimage's `resize` (output centre o
  // samples (o + 0.5) g / S - 0.5, out-of-range neighbours mirrored about the edge samples), G (S x S) scipy's
  // gaussian_filter1d (taps exp(-0.5 / sigma^2 x^2) normalised, radius int(4 sigma + 0.5), mode 'reflect').  M = G R.
  const int S = g * up;
  std::vector<double> Rm((size_t)S * g, 0.0);
  auto mirror = [g](int j) {
    if (g == 1) return 0;
    const int per = 2 * (g - 1);
    j %= per;
    if (j < 0) j += per;
    return j >= g ? per - j : j;
  };
  for (int o = 0; o < S; ++o) {
    const double c = ((double)o + 0.5) * ((double)g / (double)S) - 0.5;
    const double f = std::floor(c), w1 = c - f;
    const int j0 = (int)f;
    Rm[(size_t)o * g + mirror(j0)] += 1.0 - w1;
    Rm[(size_t)o * g + mirror(j0 + 1)] += w1;
  }
  const int rad = (int)(4.0 * sigma + 0.5);
  std::vector<double> tap(2 * rad + 1);
  double tsum = 0.0;
  for (int x = -rad; x <= rad; ++x) tsum += tap[x + rad] = std::exp(-0.5 / (sigma * sigma) * (double)(x * x));
  for (auto& t : tap) t /= tsum;
  auto reflect = [S](int j) {
    const int per = 2 * S;
    j %= per;
    if (j < 0) j += per;
    return j >= S ? per - 1 - j : j;
  };
  for (int y = 0; y < S; ++y)
    for (int j = 0; j < g; ++j) {
      double s = 0.0;
      for (int k = -rad; k <= rad; ++k) s += tap[k + rad] * Rm[(size_t)reflect(y + k) * g + j];
      M[(size_t)y * g + j] = s;
    }
  return LRP_OK;
}

int lrp_eval_expand_matrix(int32_t g, int32_t upscale, double sigma, double* M_host) {
  return guarded([&]() -> int {
    if (!M_host) return fail(LRP_ERR_INVALID, "null argument");
    if (g < 1 || g > EVAL_MAX_G || upscale < 1 || g * upscale > EVAL_MAX_S)
      return fail(LRP_ERR_INVALID, "need 1 <= g <= %d and 1 <= g * upscale <= %d", EVAL_MAX_G, EVAL_MAX_S);
    if (!(sigma > 0.0) || sigma > 1e4) return fail(LRP_ERR_INVALID, "sigma must be in (0, 1e4]");
    return eval_expand_matrix(g, upscale, sigma, M_host);
  });
}

int lrp_eval_relevance_maps(const void* R_img_dev, void* maps_dev, int32_t fp64, int32_t n, int32_t npix, int32_t C,
                            int32_t sign, void* stream) {
  return guarded([&]() -> int {
    if (!R_img_dev || !maps_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || npix < 1 || C < 1) return fail(LRP_ERR_INVALID, "n, npix, C must be positive");
    if (sign != 1 && sign != -1) return fail(LRP_ERR_INVALID, "sign must be +1 or -1");
    if (fp64 != 0 && fp64 != 1) return fail(LRP_ERR_INVALID, "fp64 must be 0 or 1");
    if (fp64)
      hipLaunchKernelGGL(eval_relevance_map_kernel<double>, dim3(n), dim3(256), 0, S(stream), (const double*)R_img_dev,
                         (double*)maps_dev, npix, C, (double)sign);
    else
      hipLaunchKernelGGL(eval_relevance_map_kernel<float>, dim3(n), dim3(256), 0, S(stream), (const float*)R_img_dev,
                         (float*)maps_dev, npix, C, (float)sign);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_eval_attention_maps(const float* att_dev, const double* M_dev, double* maps_dev, int32_t n, int32_t g, int32_t upscale,
                            void* stream) {
  return guarded([&]() -> int {
    if (!att_dev || !M_dev || !maps_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1) return fail(LRP_ERR_INVALID, "n must be positive");
    if (g < 1 || g > EVAL_MAX_G || upscale < 1 || g * upscale > EVAL_MAX_S)
      return fail(LRP_ERR_INVALID, "need 1 <= g <= %d and 1 <= g * upscale <= %d", EVAL_MAX_G, EVAL_MAX_S);
    const int Sd = g * upscale;
    const size_t lds = (size_t)(g * g + g * Sd) * sizeof(double);
    hipLaunchKernelGGL(eval_attention_map_kernel, dim3(n), dim3(256), lds, S(stream), att_dev, M_dev, maps_dev, g, Sd);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_eval_box_scores(const void* maps_dev, int32_t fp64, int32_t n, int32_t h, int32_t w, const int32_t* boxes_dev,
                        const double* thr_dev, int32_t nb, int32_t K, double* scores_dev, void* stream) {
  return guarded([&]() -> int {
    if (!maps_dev || !boxes_dev || !thr_dev || !scores_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || h < 1 || w < 1 || nb < 1) return fail(LRP_ERR_INVALID, "n, h, w, nb must be positive");
    if (K < 1 || K > EVAL_MAX_K) return fail(LRP_ERR_INVALID, "need 1 <= K <= %d thresholds", EVAL_MAX_K);
    if (fp64 != 0 && fp64 != 1) return fail(LRP_ERR_INVALID, "fp64 must be 0 or 1");
    if (fp64)
      hipLaunchKernelGGL(eval_box_score_kernel<double>, dim3(nb), dim3(256), 0, S(stream), (const double*)maps_dev, n, h, w,
                         boxes_dev, thr_dev, K, scores_dev);
    else
      hipLaunchKernelGGL(eval_box_score_kernel<float>, dim3(nb), dim3(256), 0, S(stream), (const float*)maps_dev, n, h, w,
                         boxes_dev, thr_dev, K, scores_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

// ---- Grad-CAM and the word examination (csrc/gradcam_kernels.h; explainers.py:939-949, exaimin_word.py)
int lrp_op_gradcam(const float* feat_dev, const int32_t* img_idx_dev, const float* grads_dev, const double* M_dev,
                   const float* gb_dev, double* cam_dev, double* out_dev, int32_t n, int32_t B, int32_t g, int32_t upscale,
                   int32_t D, int32_t C, void* stream) {
  return guarded([&]() -> int {
    if (!feat_dev || !img_idx_dev || !grads_dev || !M_dev || !cam_dev) return fail(LRP_ERR_INVALID, "null argument");
    if ((gb_dev == nullptr) != (out_dev == nullptr)) return fail(LRP_ERR_INVALID, "gb_dev and out_dev go together: both or neither may be null");
    if (n < 1 || B < 1) return fail(LRP_ERR_INVALID, "n and B must be positive");
    if (g < 1 || g > EVAL_MAX_G || upscale < 1 || g * upscale > EVAL_MAX_S)
      return fail(LRP_ERR_INVALID, "need 1 <= g <= %d and 1 <= g * upscale <= %d", EVAL_MAX_G, EVAL_MAX_S);
    if (D < 8 || D % 8 != 0 || D > GRADCAM_MAX_D) return fail(LRP_ERR_INVALID, "D must be a multiple of 8 in [8, %d]", GRADCAM_MAX_D);
    if (gb_dev && (C < 1 || C > 64)) return fail(LRP_ERR_INVALID, "need 1 <= C <= 64 channels of the gated map");
    const int Sd = g * upscale;
    const size_t lds = (size_t)(g * g + (D > g * Sd ? D : g * Sd)) * sizeof(double);
    hipLaunchKernelGGL(gradcam_kernel, dim3(n), dim3(256), lds, S(stream), feat_dev, img_idx_dev, grads_dev, M_dev, gb_dev,
                       cam_dev, out_dev, B, g, Sd, D, C);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_exam_maps(const void* R_img_dev, int32_t fp64, int32_t n, int32_t H, int32_t W, int32_t C, int32_t pool, int32_t k,
                  int32_t absval, void* maps_dev, double* means_dev, void* stream) {
  return guarded([&]() -> int {
    if (!R_img_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (!maps_dev && !means_dev) return fail(LRP_ERR_INVALID, "null argument: at least one of maps_dev and means_dev is needed");
    if (n < 1 || H < 1 || W < 1 || C < 1) return fail(LRP_ERR_INVALID, "n, H, W, C must be positive");
    if ((int64_t)H * W * C > INT32_MAX) return fail(LRP_ERR_INVALID, "one map must hold fewer than 2^31 values");
    if (fp64 != 0 && fp64 != 1) return fail(LRP_ERR_INVALID, "fp64 must be 0 or 1");
    if (absval != 0 && absval != 1) return fail(LRP_ERR_INVALID, "absval must be 0 or 1");
    if (pool != EXAM_POOL_NONE && pool != EXAM_POOL_MAX && pool != EXAM_POOL_AVE)
      return fail(LRP_ERR_INVALID, "pool must be 0 (none), 1 (max) or 2 (ave)");
    if (pool != EXAM_POOL_NONE && (k < 1 || H % k != 0 || W % k != 0))
      return fail(LRP_ERR_INVALID, "the pool block k must be positive and divide H and W");
    if (fp64)
      hipLaunchKernelGGL(exam_map_kernel<double>, dim3(n), dim3(256), 0, S(stream), (const double*)R_img_dev, H, W, C, pool, k,
                         absval, maps_dev, means_dev);
    else
      hipLaunchKernelGGL(exam_map_kernel<float>, dim3(n), dim3(256), 0, S(stream), (const float*)R_img_dev, H, W, C, pool, k,
                         absval, maps_dev, means_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

// ---- augment and reduce of SmoothGrad / IntegratedGradients (csrc/augment_kernels.h; innvestigate/analyzer/wrapper.py:78-345)
static int augment_rows(int32_t B, int32_t n, int64_t per_image, int32_t r0, int32_t count) {
  if (B < 1 || n < 1 || per_image < 1) return fail(LRP_ERR_INVALID, "B, n and per_image must be positive");
  if ((int64_t)B * n > INT32_MAX) return fail(LRP_ERR_INVALID, "B * n must be below 2^31");
  if (r0 < 0 || count < 1 || (int64_t)r0 + count > (int64_t)B * n)
    return fail(LRP_ERR_INVALID, "rows [%d, %lld) are not rows of the (%lld, per_image) sample matrix", r0, (long long)r0 + count,
                (long long)B * n);
  return LRP_OK;
}

int lrp_op_augment_gaussian(const float* x_dev, float* out_dev, int32_t B, int32_t n, int64_t per_image, int32_t r0, int32_t count,
                            float sigma, uint64_t seed, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    LRP_TRY(augment_rows(B, n, per_image, r0, count));
    const size_t groups = ((size_t)per_image + 3) / 4;
    hipLaunchKernelGGL(augment_gaussian_kernel, dim3(stream_grid((size_t)count * groups)), dim3(256), 0, S(stream), x_dev, out_dev, n,
                       (size_t)per_image, r0, count, sigma, (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32));
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_augment_path(const float* x_dev, const float* ref_dev, float ref_scalar, float* out_dev, int32_t B, int32_t n,
                        int64_t per_image, int32_t r0, int32_t count, int32_t mode, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (mode != 0 && mode != 1) return fail(LRP_ERR_INVALID, "mode must be 0 (the reference's x + a (x - ref)) or 1 (ref + a (x - ref))");
    LRP_TRY(augment_rows(B, n, per_image, r0, count));
    hipLaunchKernelGGL(augment_path_kernel, dim3(stream_grid((size_t)count * per_image)), dim3(256), 0, S(stream), x_dev, ref_dev,
                       ref_scalar, out_dev, n, (size_t)per_image, r0, count, mode);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_reduce_mean(int32_t phase, const float* maps_dev, double* acc_dev, int32_t B, int32_t n, int64_t per_image, int32_t r0,
                       int32_t count, int32_t post, float* out_dev, const float* x_dev, const float* ref_dev, float ref_scalar,
                       int32_t has_factor, void* stream) {
  return guarded([&]() -> int {
    if (!acc_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (phase == 0) {
      if (!maps_dev) return fail(LRP_ERR_INVALID, "null argument");
      if (post != AUG_POST_NONE && post != AUG_POST_ABS && post != AUG_POST_SQUARE)
        return fail(LRP_ERR_INVALID, "post must be 0 (none), 1 (abs) or 2 (square)");
      LRP_TRY(augment_rows(B, n, per_image, r0, count));
      const size_t imgs = (size_t)((r0 + count - 1) / n - r0 / n + 1);
      hipLaunchKernelGGL(reduce_accum_kernel, dim3(stream_grid(imgs * per_image)), dim3(256), 0, S(stream), maps_dev, acc_dev, n,
                         (size_t)per_image, r0, count, post);
    } else if (phase == 1) {
      if (!out_dev) return fail(LRP_ERR_INVALID, "null argument");
      if (B < 1 || n < 1 || per_image < 1) return fail(LRP_ERR_INVALID, "B, n and per_image must be positive");
      if (has_factor != 0 && has_factor != 1) return fail(LRP_ERR_INVALID, "has_factor must be 0 or 1");
      if (has_factor && !x_dev) return fail(LRP_ERR_INVALID, "the factor x - ref needs x_dev");
      const size_t total = (size_t)B * per_image;
      hipLaunchKernelGGL(reduce_finish_kernel, dim3(stream_grid(total)), dim3(256), 0, S(stream), acc_dev, out_dev, n, total, has_factor,
                         x_dev, ref_dev, ref_scalar);
    } else {
      return fail(LRP_ERR_INVALID, "phase must be 0 (accumulate) or 1 (finish)");
    }
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

// ---- perturbation analysis (csrc/perturb_kernels.h; innvestigate/tools/perturbate.py)
// The geometry of PT:105-116 / PT:170: no padding when the region divides both axes, r - dim % r per axis (floor(pad / 2)
// before) when it divides neither; one divisible axis is the reference's assert at PT:107.
static int perturb_geometry(int32_t H, int32_t W, int32_t C, int32_t rh, int32_t rw, PerturbGeom* g) {
  if (H < 1 || W < 1 || C < 1) return fail(LRP_ERR_INVALID, "H, W, C must be positive");
  if ((int64_t)H * W * C > INT32_MAX) return fail(LRP_ERR_INVALID, "one map must hold fewer than 2^31 values");
  if (rh < 1 || rw < 1) return fail(LRP_ERR_RANGE, "the region shape must be at least 1 x 1");
  if (rh > (1 << 15) || rw > (1 << 15)) return fail(LRP_ERR_RANGE, "a region side may not exceed 32768");
  const bool dh = H % rh == 0, dw = W % rw == 0;
  if (dh != dw)
    return fail(LRP_ERR_INVALID, "region (%d, %d) divides one axis of (%d, %d) and not the other: the reference pads the "
                "divisible axis by a whole region and fails its assert (perturbate.py:107)", rh, rw, H, W);
  const int ph = dh ? 0 : rh - H % rh, pw = dw ? 0 : rw - W % rw;
  const int64_t nreg = (int64_t)((H + ph) / rh) * ((W + pw) / rw);
  if (nreg > PERTURB_MAX_REGIONS) return fail(LRP_ERR_RANGE, "%lld regions: at most %d are ranked", (long long)nreg, PERTURB_MAX_REGIONS);
  *g = PerturbGeom{H, W, C, rh, rw, (H + ph) / rh, (W + pw) / rw, ph / 2, pw / 2};
  return LRP_OK;
}

int lrp_perturb_ranks(const void* R_img_dev, int32_t fp64, int32_t n, int32_t H, int32_t W, int32_t C, int32_t rh, int32_t rw,
                      int32_t reduce, int32_t aggregate, int32_t negate, int32_t* ranks_dev, double* scores_dev, void* stream) {
  return guarded([&]() -> int {
    if (!R_img_dev || !ranks_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1) return fail(LRP_ERR_INVALID, "n must be positive");
    if (fp64 != 0 && fp64 != 1) return fail(LRP_ERR_INVALID, "fp64 must be 0 or 1");
    if (negate != 0 && negate != 1) return fail(LRP_ERR_INVALID, "negate must be 0 or 1");
    if ((reduce != PERTURB_FN_MEAN && reduce != PERTURB_FN_MAX) || (aggregate != PERTURB_FN_MEAN && aggregate != PERTURB_FN_MAX))
      return fail(LRP_ERR_INVALID, "reduce and aggregate must be 0 (mean) or 1 (max)");
    PerturbGeom g;
    LRP_TRY(perturb_geometry(H, W, C, rh, rw, &g));
    const size_t lds = (size_t)g.Hr * g.Wr * sizeof(double);
    const double sign = negate ? -1.0 : 1.0;
    if (fp64)
      hipLaunchKernelGGL(perturb_rank_kernel<double>, dim3(n), dim3(256), lds, S(stream), (const double*)R_img_dev, g, reduce,
                         aggregate, sign, ranks_dev, scores_dev);
    else
      hipLaunchKernelGGL(perturb_rank_kernel<float>, dim3(n), dim3(256), lds, S(stream), (const float*)R_img_dev, g, reduce,
                         aggregate, sign, ranks_dev, scores_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_perturb_apply(const float* x_dev, const int32_t* img_idx_dev, const int32_t* ranks_dev, const double* k_dev,
                      const float* noise_dev, float* out_dev, int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t rh,
                      int32_t rw, int32_t mode, int32_t all_channels, int32_t has_range, float lo, float hi, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !img_idx_dev || !ranks_dev || !k_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || B < 1) return fail(LRP_ERR_INVALID, "n and B must be positive");
    if (mode != PERTURB_ZEROS && mode != PERTURB_MEAN && mode != PERTURB_INVERT && mode != PERTURB_NOISE)
      return fail(LRP_ERR_INVALID, "mode must be 0 (zeros), 1 (mean), 2 (invert) or 3 (noise)");
    if ((mode == PERTURB_NOISE) != (noise_dev != nullptr)) return fail(LRP_ERR_INVALID, "noise_dev goes with mode 3 (noise) and with no other");
    if ((all_channels != 0 && all_channels != 1) || (has_range != 0 && has_range != 1))
      return fail(LRP_ERR_INVALID, "all_channels and has_range must be 0 or 1");
    if (has_range && !(lo <= hi)) return fail(LRP_ERR_INVALID, "the value range needs lo <= hi");
    PerturbGeom g;
    LRP_TRY(perturb_geometry(H, W, C, rh, rw, &g));
    hipLaunchKernelGGL(perturb_apply_kernel, dim3(n), dim3(256), 0, S(stream), x_dev, img_idx_dev, ranks_dev, k_dev, noise_dev,
                       out_dev, B, g, mode, all_channels, has_range, lo, hi);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_perturb_word_scores(lrp_handle* h, const int32_t* slot_dev, const int32_t* t_dev, const int32_t* k_dev, int32_t n,
                            double* logit_dev, double* logp_dev, void* stream) {
  return with_handle(h, [&]() -> int {
    if (!h || !slot_dev || !t_dev || !k_dev || !logit_dev || !logp_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1) return fail(LRP_ERR_INVALID, "n must be positive");
    if (!h->dec.have_forward) return fail(LRP_ERR_STATE, "lrp_decoder_forward must run before lrp_perturb_word_scores");
    hipLaunchKernelGGL(perturb_word_score_kernel, dim3(n), dim3(256), 0, S(stream), h->dec.S_<double>("caption_preds"), slot_dev,
                       t_dev, k_dev, h->dec.B_cur, h->dec.Tm, h->dec.V, logit_dev, logp_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}


// ---- occlusion and RISE word saliency (csrc/saliency_kernels.h)
static int saliency_image(int32_t H, int32_t W, int32_t C) {
  if (H < 1 || W < 1 || C < 1) return fail(LRP_ERR_INVALID, "H, W, C must be positive");
  if ((int64_t)H * W * C > INT32_MAX) return fail(LRP_ERR_INVALID, "one image must hold fewer than 2^31 values");
  return LRP_OK;
}

static int occlusion_geometry(int32_t H, int32_t W, int32_t C, int32_t ph, int32_t pw, int32_t sh, int32_t sw, OccGeom* g) {
  LRP_TRY(saliency_image(H, W, C));
  if (sh < 1 || sh > ph || ph > H || sw < 1 || sw > pw || pw > W)
    return fail(LRP_ERR_INVALID, "occlusion needs 1 <= stride <= window <= image on both axes: window (%d, %d), stride (%d, %d), "
                "image (%d, %d)", ph, pw, sh, sw, H, W);
  const int64_t Hn = (H - ph + sh - 1) / sh + 1, Wn = (W - pw + sw - 1) / sw + 1;
  if (Hn * Wn > OCC_MAX_WINDOWS) return fail(LRP_ERR_RANGE, "%lld windows: at most %d are scored", (long long)(Hn * Wn), OCC_MAX_WINDOWS);
  *g = OccGeom{H, W, C, ph, pw, sh, sw, (int)Hn, (int)Wn};
  return LRP_OK;
}

static int rise_geometry(int32_t H, int32_t W, int32_t C, int32_t s, int32_t ch, int32_t cw, RiseGeom* g) {
  LRP_TRY(saliency_image(H, W, C));
  if (s < 1 || s > RISE_MAX_S) return fail(LRP_ERR_RANGE, "RISE grid s=%d outside [1,%d]", s, RISE_MAX_S);
  if (ch < (H + s - 1) / s || cw < (W + s - 1) / s)
    return fail(LRP_ERR_INVALID, "RISE cell (%d, %d) is below (ceil(H / s), ceil(W / s)) = (%d, %d): the grid would not cover the image",
                ch, cw, (H + s - 1) / s, (W + s - 1) / s);
  if (ch > RISE_MAX_CELL || cw > RISE_MAX_CELL) return fail(LRP_ERR_INVALID, "a RISE cell side may not exceed %d", RISE_MAX_CELL);
  *g = RiseGeom{H, W, C, s, ch, cw};
  return LRP_OK;
}

static int rise_probability(double p) {
  if (!(p > 0.0) || !(p <= 1.0)) return fail(LRP_ERR_INVALID, "RISE needs 0 < p <= 1 (p=%g)", p);
  return LRP_OK;
}

static bool aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

int lrp_op_occlude(const float* x_dev, const int32_t* img_idx_dev, const int32_t* k_dev, const float* fill_dev, float* out_dev,
                   int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ph, int32_t pw, int32_t sh, int32_t sw,
                   void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !img_idx_dev || !k_dev || !fill_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || B < 1) return fail(LRP_ERR_INVALID, "n and B must be positive");
    OccGeom g;
    LRP_TRY(occlusion_geometry(H, W, C, ph, pw, sh, sw, &g));
    const size_t per = (size_t)H * W * C, work = (size_t)n * ((per + 3) / 4);
    if (per % 4 == 0 && aligned16(x_dev, out_dev))
      hipLaunchKernelGGL(occlude_kernel<true>, dim3(stream_grid(work)), dim3(256), 0, S(stream), x_dev, img_idx_dev, k_dev, fill_dev,
                         out_dev, n, B, g);
    else
      hipLaunchKernelGGL(occlude_kernel<false>, dim3(stream_grid(work)), dim3(256), 0, S(stream), x_dev, img_idx_dev, k_dev, fill_dev,
                         out_dev, n, B, g);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_occlusion_map(const double* scores_dev, float* out_dev, int32_t n_img, int32_t T, int32_t H, int32_t W, int32_t ph,
                         int32_t pw, int32_t sh, int32_t sw, void* stream) {
  return guarded([&]() -> int {
    if (!scores_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n_img < 1 || T < 1) return fail(LRP_ERR_INVALID, "n_img and T must be positive");
    OccGeom g;
    LRP_TRY(occlusion_geometry(H, W, 1, ph, pw, sh, sw, &g));
    hipLaunchKernelGGL(occlusion_map_kernel, dim3(stream_grid((size_t)n_img * T * H * W)), dim3(256), 0, S(stream), scores_dev,
                       out_dev, n_img, T, g);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_rise_grids(const uint32_t* key_dev, const int32_t* k_dev, int32_t n, int32_t s, double p, uint64_t seed, int32_t H,
                      int32_t W, int32_t ch, int32_t cw, uint8_t* grid_dev, int32_t* shift_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key_dev || !k_dev || !grid_dev || !shift_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1) return fail(LRP_ERR_INVALID, "n must be positive");
    RiseGeom g;
    LRP_TRY(rise_geometry(H, W, 1, s, ch, cw, &g));
    LRP_TRY(rise_probability(p));
    const unsigned thresh = (unsigned)std::floor(p * 16777216.0);
    const size_t work = (size_t)n * (((size_t)(s + 1) * (s + 1) + 3) / 4 + 1);
    hipLaunchKernelGGL(rise_grids_kernel, dim3(stream_grid(work)), dim3(256), 0, S(stream), key_dev, k_dev, n, s, thresh,
                       (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), ch, cw, grid_dev, shift_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_rise_apply(const float* x_dev, const int32_t* img_idx_dev, const uint8_t* grid_dev, const int32_t* shift_dev,
                      const float* fill_dev, float* out_dev, int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s,
                      int32_t ch, int32_t cw, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !img_idx_dev || !grid_dev || !shift_dev || !fill_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || B < 1) return fail(LRP_ERR_INVALID, "n and B must be positive");
    RiseGeom g;
    LRP_TRY(rise_geometry(H, W, C, s, ch, cw, &g));
    const size_t per = (size_t)H * W * C, work = (size_t)n * ((per + 3) / 4);
    if (per % 4 == 0 && aligned16(x_dev, out_dev))
      hipLaunchKernelGGL(rise_apply_kernel<true>, dim3(stream_grid(work)), dim3(256), 0, S(stream), x_dev, img_idx_dev, grid_dev,
                         shift_dev, fill_dev, out_dev, n, B, g);
    else
      hipLaunchKernelGGL(rise_apply_kernel<false>, dim3(stream_grid(work)), dim3(256), 0, S(stream), x_dev, img_idx_dev, grid_dev,
                         shift_dev, fill_dev, out_dev, n, B, g);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_rise_map(const double* scores_dev, const uint8_t* grid_dev, const int32_t* shift_dev, float* out_dev, int32_t n_img,
                    int32_t K, int32_t T, int32_t H, int32_t W, int32_t s, double p, int32_t ch, int32_t cw, void* stream) {
  return guarded([&]() -> int {
    if (!scores_dev || !grid_dev || !shift_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n_img < 1 || K < 1 || T < 1) return fail(LRP_ERR_INVALID, "n_img, K and T must be positive");
    RiseGeom g;
    LRP_TRY(rise_geometry(H, W, 1, s, ch, cw, &g));
    LRP_TRY(rise_probability(p));
    const int64_t blocks = (int64_t)n_img * ((T + RISE_TT - 1) / RISE_TT) * (((int64_t)H * W + 255) / 256);
    if (blocks > INT32_MAX) return fail(LRP_ERR_INVALID, "n_img * T * H * W is too large for one launch: split the images");
    hipLaunchKernelGGL(rise_map_kernel, dim3((unsigned)blocks), dim3(256), 0, S(stream), scores_dev, grid_dev, shift_dev, out_dev, K, T,
                       g, (double)K * p);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

// ---- the CAM family as word saliencies (csrc/cam_kernels.h)
static int cam_geometry(int32_t g, int32_t upscale, int32_t D) {
  if (g < 1 || g > EVAL_MAX_G || upscale < 1 || g * upscale > EVAL_MAX_S)
    return fail(LRP_ERR_INVALID, "need 1 <= g <= %d and 1 <= g * upscale <= %d", EVAL_MAX_G, EVAL_MAX_S);
  if (D < 8 || D % 8 != 0 || D > GRADCAM_MAX_D) return fail(LRP_ERR_INVALID, "D must be a multiple of 8 in [8, %d]", GRADCAM_MAX_D);
  return LRP_OK;
}

int lrp_op_cam(const float* feat_dev, const int32_t* img_idx_dev, const float* grads_dev, const double* M_dev, const float* gb_dev,
               double* cam_dev, double* out_dev, int32_t n, int32_t B, int32_t g, int32_t upscale, int32_t D, int32_t C,
               int32_t mode, void* stream) {
  return guarded([&]() -> int {
    if (!feat_dev || !img_idx_dev || !grads_dev || !M_dev || !cam_dev) return fail(LRP_ERR_INVALID, "null argument");
    if ((gb_dev == nullptr) != (out_dev == nullptr)) return fail(LRP_ERR_INVALID, "gb_dev and out_dev go together: both or neither may be null");
    if (n < 1 || B < 1) return fail(LRP_ERR_INVALID, "n and B must be positive");
    LRP_TRY(cam_geometry(g, upscale, D));
    if (gb_dev && (C < 1 || C > 64)) return fail(LRP_ERR_INVALID, "need 1 <= C <= 64 channels of the gated map");
    if (mode < 0 || mode >= CAM_MODES)
      return fail(LRP_ERR_INVALID, "mode must be 0 (gradcam), 1 (gradcam++), 2 (xgradcam), 3 (layercam) or 4 (hirescam)");
    const int Sd = g * upscale;
    const size_t lds = (size_t)(g * g + (D > g * Sd ? D : g * Sd)) * sizeof(double);
    hipLaunchKernelGGL(cam_kernel, dim3(n), dim3(256), lds, S(stream), feat_dev, img_idx_dev, grads_dev, M_dev, gb_dev, cam_dev,
                       out_dev, B, g, Sd, D, C, mode);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_cam_weighted(const double* scores_dev, const float* feat_dev, const int32_t* img_idx_dev, const double* M_dev,
                        double* cam_dev, float* map_dev, int32_t n_img, int32_t R, int32_t T, int32_t B, int32_t g, int32_t upscale,
                        int32_t D, int32_t mode, void* stream) {
  return guarded([&]() -> int {
    if (!scores_dev || !feat_dev || !img_idx_dev || !M_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (!cam_dev && !map_dev) return fail(LRP_ERR_INVALID, "null argument: at least one of cam_dev and map_dev is needed");
    if (n_img < 1 || T < 1 || B < 1) return fail(LRP_ERR_INVALID, "n_img, T and B must be positive");
    LRP_TRY(cam_geometry(g, upscale, D));
    if (mode < 0 || mode >= CAMW_MODES) return fail(LRP_ERR_INVALID, "mode must be 0 (softmax), 1 (linear) or 2 (ablation)");
    const int rows = 1 + D + (mode == CAMW_LINEAR ? 1 : 0);
    if (R != rows) return fail(LRP_ERR_INVALID, "the scores need R = %d rows per image in this mode (R=%d)", rows, R);
    if ((int64_t)n_img * T > INT32_MAX) return fail(LRP_ERR_INVALID, "n_img * T must be below 2^31");
    const int Sd = g * upscale;
    const size_t lds = (size_t)(g * g + (D > g * Sd ? D : g * Sd)) * sizeof(double);
    hipLaunchKernelGGL(cam_weighted_kernel, dim3(n_img * T), dim3(256), lds, S(stream), scores_dev, feat_dev, img_idx_dev, M_dev,
                       cam_dev, map_dev, B, R, T, g, Sd, D, mode);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_scorecam_apply(const float* x_dev, const float* feat_dev, const int32_t* img_idx_dev, const int32_t* k_dev,
                          const float* fill_dev, float* out_dev, int32_t n, int32_t B, int32_t g, int32_t upscale, int32_t C,
                          int32_t D, void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !feat_dev || !img_idx_dev || !k_dev || !fill_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || n > 65535 || B < 1) return fail(LRP_ERR_INVALID, "need 1 <= n <= 65535 rows and a positive B");
    if (g < 1 || g > EVAL_MAX_G || upscale < 1 || upscale > RISE_MAX_CELL)
      return fail(LRP_ERR_INVALID, "need 1 <= g <= %d and 1 <= upscale <= %d", EVAL_MAX_G, RISE_MAX_CELL);
    if (D < 1) return fail(LRP_ERR_INVALID, "D must be positive");
    if ((int64_t)g * upscale > INT32_MAX) return fail(LRP_ERR_INVALID, "one image must hold fewer than 2^31 values");
    const int Sd = g * upscale;
    LRP_TRY(saliency_image(Sd, Sd, C));
    const size_t per = (size_t)Sd * Sd * C, groups = (per + 3) / 4;
    const dim3 grid((unsigned)((groups + CAM_SLICE - 1) / CAM_SLICE), (unsigned)n);
    const ScoreCamGeom q{g, upscale, C, D};
    if (per % 4 == 0 && aligned16(x_dev, out_dev))
      hipLaunchKernelGGL(scorecam_apply_kernel<true>, grid, dim3(256), 0, S(stream), x_dev, feat_dev, img_idx_dev, k_dev, fill_dev,
                         out_dev, B, q);
    else
      hipLaunchKernelGGL(scorecam_apply_kernel<false>, grid, dim3(256), 0, S(stream), x_dev, feat_dev, img_idx_dev, k_dev, fill_dev,
                         out_dev, B, q);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_feature_ablate(const float* feat_dev, const int32_t* img_idx_dev, const int32_t* k_dev, float* out_dev, int32_t n,
                          int32_t B, int32_t L, int32_t D, void* stream) {
  return guarded([&]() -> int {
    if (!feat_dev || !img_idx_dev || !k_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || B < 1 || L < 1 || D < 1) return fail(LRP_ERR_INVALID, "n, B, L and D must be positive");
    if ((int64_t)L * D > INT32_MAX) return fail(LRP_ERR_INVALID, "one feature map must hold fewer than 2^31 values");
    const size_t per = (size_t)L * D, work = (size_t)n * ((per + 3) / 4);
    if (per % 4 == 0 && aligned16(feat_dev, out_dev))
      hipLaunchKernelGGL(feature_ablate_kernel<true>, dim3(stream_grid(work)), dim3(256), 0, S(stream), feat_dev, img_idx_dev, k_dev,
                         out_dev, n, B, L, D);
    else
      hipLaunchKernelGGL(feature_ablate_kernel<false>, dim3(stream_grid(work)), dim3(256), 0, S(stream), feat_dev, img_idx_dev, k_dev,
                         out_dev, n, B, L, D);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

// ---- LIME and KernelSHAP word saliency (csrc/segment_kernels.h)
static int segment_count(int32_t d) {
  if (d < 2 || d > SEG_MAX_D) return fail(LRP_ERR_RANGE, "segment count d=%d outside [2,%d]", d, SEG_MAX_D);
  return LRP_OK;
}

int lrp_op_segment_draws(const uint32_t* key_dev, const int32_t* k_dev, int32_t n, int32_t d, int32_t mode, double p,
                         const uint32_t* thr_dev, uint64_t seed, uint32_t* bits_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key_dev || !k_dev || !bits_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1) return fail(LRP_ERR_INVALID, "n must be positive");
    LRP_TRY(segment_count(d));
    if (mode != LRP_SEGMENT_BERNOULLI && mode != LRP_SEGMENT_SHAPLEY) return fail(LRP_ERR_INVALID, "unknown draw mode %d", mode);
    unsigned thresh = 0;
    if (mode == LRP_SEGMENT_BERNOULLI) {
      if (!(p > 0.0) || !(p <= 1.0)) return fail(LRP_ERR_INVALID, "Bernoulli draws need 0 < p <= 1 (p=%g)", p);
      thresh = (unsigned)std::floor(p * 16777216.0);
    } else if (d > 2 && !thr_dev) {
      return fail(LRP_ERR_INVALID, "Shapley draws at d > 2 need the d - 2 size thresholds");
    }
    hipLaunchKernelGGL(segment_draws_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)n + SEG_DRAW_THREADS - 1) / SEG_DRAW_THREADS, 4096)),
                       dim3(SEG_DRAW_THREADS), 0, S(stream), key_dev, k_dev, n, d, mode == LRP_SEGMENT_SHAPLEY ? 1 : 0, thresh, thr_dev,
                       (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), bits_dev);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_segment_apply(const float* x_dev, const int32_t* img_idx_dev, const uint32_t* bits_dev, const int32_t* label_dev,
                         const float* fill_dev, float* out_dev, int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t d,
                         void* stream) {
  return guarded([&]() -> int {
    if (!x_dev || !img_idx_dev || !bits_dev || !label_dev || !fill_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n < 1 || B < 1) return fail(LRP_ERR_INVALID, "n and B must be positive");
    LRP_TRY(saliency_image(H, W, C));
    LRP_TRY(segment_count(d));
    const size_t per = (size_t)H * W * C, work = (size_t)n * ((per + 3) / 4);
    if (per % 4 == 0 && aligned16(x_dev, out_dev))
      hipLaunchKernelGGL(segment_apply_kernel<true>, dim3(stream_grid(work)), dim3(256), 0, S(stream), x_dev, img_idx_dev, bits_dev,
                         label_dev, fill_dev, out_dev, n, B, H, W, C, d);
    else
      hipLaunchKernelGGL(segment_apply_kernel<false>, dim3(stream_grid(work)), dim3(256), 0, S(stream), x_dev, img_idx_dev, bits_dev,
                         label_dev, fill_dev, out_dev, n, B, H, W, C, d);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_segment_fit(const uint32_t* bits_dev, const double* wtab_dev, const double* y_dev, const double* delta_dev, double ridge,
                       double* phi_dev, double* icpt_dev, int32_t* status_dev, int32_t n_img, int32_t K, int32_t T, int32_t d,
                       void* stream) {
  return guarded([&]() -> int {
    if (!bits_dev || !wtab_dev || !y_dev || !phi_dev || !icpt_dev || !status_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n_img < 1 || K < 1 || T < 1) return fail(LRP_ERR_INVALID, "n_img, K and T must be positive");
    LRP_TRY(segment_count(d));
    if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(LRP_ERR_INVALID, "ridge must be finite and >= 0 (ridge=%g)", ridge);
    const size_t lds = segment_fit_lds(delta_dev ? d - 1 : d + 1);
    // above the 64 KiB a kernel may take unasked, the dynamic-LDS attribute is raised once, to the largest case (d = SEG_MAX_D)
    static std::atomic<bool> attr_set{false};
    if (lds > 64 * 1024 && !attr_set.load()) {
      LRP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(segment_fit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)segment_fit_lds(SEG_MAX_D + 1)));
      attr_set.store(true);
    }
    hipLaunchKernelGGL(segment_fit_kernel, dim3((unsigned)n_img), dim3(SEG_FIT_THREADS), lds, S(stream), bits_dev, wtab_dev, y_dev,
                       delta_dev, ridge, phi_dev, icpt_dev, status_dev, K, T, d);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

int lrp_op_segment_map(const double* phi_dev, const int32_t* label_dev, float* out_dev, int32_t n_img, int32_t T, int32_t H,
                       int32_t W, int32_t d, void* stream) {
  return guarded([&]() -> int {
    if (!phi_dev || !label_dev || !out_dev) return fail(LRP_ERR_INVALID, "null argument");
    if (n_img < 1 || T < 1) return fail(LRP_ERR_INVALID, "n_img and T must be positive");
    LRP_TRY(saliency_image(H, W, 1));
    LRP_TRY(segment_count(d));
    hipLaunchKernelGGL(segment_map_kernel, dim3(stream_grid((size_t)n_img * T * H * W)), dim3(256), 0, S(stream), phi_dev, label_dev,
                       out_dev, n_img, T, H, W, d);
    LRP_HIP_CHECK(hipGetLastError());
    return LRP_OK;
  });
}

}  // extern "C"
