/* lrp_hip.h — C ABI of the MI355X-native LRP engine (liblrp_hip.so).
 *
 * Drop-in boundary for the explanation hot path of SunJiamei/LRP-ImageCaptioning.
 * The reference is pure Python and has no FFI; each entry point below names the
 * reference call it stands in for (file:line in /root/reference; E: =
 * models/explainers.py, AB: = innvestigate/analyzer/base.py, RA:/RR: =
 * innvestigate/analyzer/relevance_based/relevance_{analyzer,rule}.py).
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C types only; every `*_dev` pointer is DEVICE memory owned by the
 *    caller (e.g. a torch tensor's data_ptr()); every `*_host` pointer is host
 *    memory read before the call returns.
 *  - the library allocates only its own workspace, freed in lrp_destroy: the
 *    caches and walk buffers in lrp_create, operand copies in lrp_set_weight[_dev],
 *    the trainer's state in lrp_train_begin; a few buffers whose need depends on
 *    which entry points a caller uses (decoder scan / gradient operand packs,
 *    per-token scale records of the fp16 fast mode, per-gate dropout products)
 *    are allocated by the FIRST call that needs them and kept.  A compute call
 *    never synchronises the device or a stream; the host side may wait on an
 *    event for the PREVIOUS call's small pinned staging copy (index arrays, the
 *    tile-order table of a reverse-walk launch) before reusing that buffer.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *  - return value: 0 = LRP_OK, negative = error; text via lrp_last_error().
 *  - one handle per GPU / stream; a handle is stateful and not re-entrant
 *    (like the reference engine, whose state lives on `self`).
 *  - tensors are row-major, images / feature maps NHWC (Keras channels_last),
 *    dense weights (in_dim, out_dim), conv kernels HWIO, LSTM gate order i,f,g,o
 *    — exactly the arrays `layer.get_weights()` yields at E:264-278 / E:1000-1019.
 */
#ifndef LRP_HIP_H
#define LRP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRP_ABI_VERSION 10

enum {
  LRP_OK = 0,
  LRP_ERR_INVALID = -1,      /* bad argument (ValueError at the Python layer)          */
  LRP_ERR_STATE = -2,        /* call order violated / weights missing                  */
  LRP_ERR_HIP = -3,          /* a HIP runtime call failed                              */
  LRP_ERR_NOMEM = -4,        /* workspace allocation failed                            */
  LRP_ERR_RANGE = -5,        /* token index out of range of the caption
                                (NotImplementedError at E:538-539 / E:1181-1182)       */
  LRP_ERR_UNSUPPORTED = -6   /* encoder/decoder kind not built (NotImplementedError)   */
};

enum { LRP_DEC_ADAPTIVE = 0,   /* ExplainImgCaptioningAdaptiveAttention  E:260-666   */
       LRP_DEC_GRIDTD = 1 };   /* ExplainImgCaptioningGridTDModel        E:995-1321  */

enum { LRP_EXPLAIN_SEQUENCE = 0,   /* _explain_lstm_single_word_sequence  E:537-666 / E:1180-1321 */
       LRP_EXPLAIN_SINGLE_STEP = 1 /* _explain_lstm_single_word           E:438-535 (adaptive)    */ };

enum { LRP_ENC_VGG = 0, LRP_ENC_RESNET = 1 };

#define LRP_MAX_CONV 32

/* Encoder = a VGG-style stack cut after the last conv's ReLU (the sub-model
 * input_1 -> block5_conv3 of E:29-30): conv3x3 'same' + ReLU layers, each
 * optionally followed by a 2x2/2 max-pool.  VGG16: 13 convs, pools after
 * 2,4,7,10.  conv_name[i] is the Keras layer name used by lrp_set_weight
 * ("<name>_W" HWIO (3,3,Cin,Cout), "<name>_b" (Cout)). */
typedef struct lrp_config {
  int32_t abi_version;          /* = LRP_ABI_VERSION                                    */
  int32_t device;               /* HIP device ordinal                                   */
  int32_t decoder;              /* LRP_DEC_*                                            */
  int32_t img_h, img_w;         /* 224, 224.  img_h != img_w is supported by both encoders, every walk and the
                                   fine-tune step (tests/test_gpu_nonsquare.py).  lrp_create refuses with
                                   LRP_ERR_UNSUPPORTED: VGG-style, an odd resolution in front of a 2x2 pool; ResNet,
                                   sides that are not multiples of 4 or an odd resolution in front of a stride-2
                                   block.  L = (top rows) x (top columns), row-major.                            */
  int32_t n_conv;
  int32_t conv_cin[LRP_MAX_CONV];
  int32_t conv_cout[LRP_MAX_CONV];
  int32_t conv_pool_after[LRP_MAX_CONV];
  char    conv_name[LRP_MAX_CONV][32];
  int32_t L, D, H, E, V;        /* 196, 512, 512, 512, vocab  (config.py:14-15,36-40);  D, H multiples of 8;
                                   E >= 4, any width with 2E + 2H <= 2048, E != H included (LRP, forward replay and
                                   caption generation read every 2E-strided row with scalar loads).  E == H is needed
                                   by lrp_train_begin and by the ADAPTIVE lrp_decoder_gradient, E % 4 == 0 (and
                                   D, H % 4) by every lrp_decoder_gradient */
  int32_t max_images;           /* capacity of the per-image caches                     */
  int32_t max_tokens;           /* capacity of one explain call (heat-maps)             */
  int32_t max_caption_len;      /* longest caption incl. EOS (config.py:34 -> 20+1)     */
  int32_t sos_id, eos_id;       /* tokenizer ids (1-based); model column = id-1 (E:443) */
  /* ABI v2: encoder selection.  LRP_ENC_VGG uses the conv_* table above.  LRP_ENC_RESNET builds the Keras
   * ResNet-v1 bottleneck encoder (keras_applications.resnet_common; ResNet-101 = stem 64, filters 64/128/256/512,
   * blocks 3/4/23/3) cut after the last block's ReLU (conv5_block3_out, config.py:41-45); weights are named
   * "<unit>_conv_W" HWIO, "<unit>_conv_b", "<unit>_bn_gamma|beta|mean|var" with <unit> = "conv1" or
   * "conv<s>_block<b>_<0|1|2|3>" (0 = projection shortcut).  The conv_* table is ignored. */
  int32_t encoder;              /* LRP_ENC_VGG / LRP_ENC_RESNET                         */
  int32_t resnet_stem;          /* 64                                                   */
  int32_t resnet_n_stacks;      /* 4                                                    */
  int32_t resnet_filters[8];    /* 64,128,256,512                                       */
  int32_t resnet_blocks[8];     /* 3,4,23,3                                             */
} lrp_config;

typedef struct lrp_handle lrp_handle;

/* ExplainImgCaptioningAttentionModel.__init__ (E:24-40): build the engine for a
 * model geometry; allocates all device workspace.  LRP_ERR_UNSUPPORTED when D or
 * H is not a multiple of 8, or 2E+2H > 2048. */
int lrp_create(const lrp_config* cfg, lrp_handle** out);
int lrp_destroy(lrp_handle* h);

/* Weight extraction (E:264-278, E:1000-1019; conv kernels = the image_model's
 * layers, E:29-30).  `data_host` is float32 in the Keras layout; the library
 * copies the array into HBM and builds every operand copy there (conv weights
 * split into w+ / w-, RR:256-260) with the packers of lrp_set_weight_dev —
 * there is one packing route.  Synchronous: on return the array has been read
 * and may be reused or freed.  An encoder weight invalidates the encode caches
 * (lrp_encode_images must run again before an explain call).
 * Names: "<conv>_W","<conv>_b", "image_features_W/_b", "global_W/_b",
 * "embedding", "output_W/_b"; adaptive: "lstm_Wi","lstm_Wh","lstm_b","Wv","Wg",
 * "V","Wx","Wh","Ws"; grid-TD: "td_Wi","td_Wh","td_b","lang_Wi","lang_Wh",
 * "lang_b","W_va","W_ha","W_a","W_x","W_h","W_s". */
int lrp_set_weight(lrp_handle* h, const char* name, const float* data_host,
                   int32_t ndim, const int64_t* shape);
/* Same, from device memory on rank-local HBM (used after an RCCL broadcast).  ABI v3: packed by device kernels — a
 * device-to-device copy of the array plus the pack / split kernels on `stream`; no host round trip and no stream
 * synchronisation, for the conv-list (VGG) encoder, both decoders and (ABI v4) the ResNet encoder's units
 * ("<unit>_conv_W/_conv_b/_bn_gamma/_bn_beta/_bn_mean/_bn_var") alike.  The caller's buffer is copied before the call
 * returns control to the stream's next work, so it may be released (stream-ordered) right after.  Host-set and device-set
 * weights may be mixed; the last setter of a name wins. */
int lrp_set_weight_dev(lrp_handle* h, const char* name, const float* data_dev,
                       int32_t ndim, const int64_t* shape, void* stream);

/* `self._image_model.predict(img_input)` (E:375, E:1097) plus everything the
 * analyzer's forward half would recompute on every analyze() call (AB:511):
 * runs the encoder once per image and caches, per conv layer, the relevance
 * gate G_l = argmax_mask_l * a_l / SafeDivide-denominator(Z+_l) (RR:274-322,
 * layers.py:446-461) and the top feature map.  images_dev: (B,img_h,img_w,3)
 * float32, BGR mean-subtracted (preprocessors.py:43-44). */
int lrp_encode_images(lrp_handle* h, const float* images_dev, int32_t B, void* stream);

/* Decoder-only use (parity tests of the E: classes with an injected feature
 * map, mirroring a stubbed `_image_model.predict`): features_dev (B,L,D). */
int lrp_set_features(lrp_handle* h, const float* features_dev, int32_t B, void* stream);
/* Copy out the cached top feature map (B,L,D). */
int lrp_get_features(lrp_handle* h, float* features_dev, int32_t B, void* stream);

/* _forward_beam_search(X, caption) (E:370-436 / E:1092-1178) for B images at
 * once: teacher-forced replay, caches ht, ct, gt, it_act, ft_act, context,
 * attention, st, beta, c_hat, xt, caption_preds on the handle.
 * captions_host: (B, max_caption_len) tokenizer ids, row b valid for
 * lengths_host[b] entries (last valid one = EOS). */
int lrp_decoder_forward(lrp_handle* h, const int32_t* captions_host,
                        const int32_t* lengths_host, int32_t B, void* stream);

/* Read a cached decoder state array (the attributes the reference leaves on
 * `self`).  Layout (B, max_caption_len+1, dim) with row 0 = zero init, float32
 * for ht/ct/gt/it_act/ft_act/st/attention/beta, float64 for context/c_hat;
 * "caption_preds" (B, max_caption_len, V) float64; "xt" (B, max_caption_len, 2E).
 * grid-TD: h1t,c1t,g1t,i1t_act,f1t_act,h2t,c2t,g2t,i2t_act,f2t_act, context,
 * st, beta, context_hat, attention (float64 where the reference has float64). */
int lrp_read_state(lrp_handle* h, const char* name, void* out_dev, size_t out_bytes, void* stream);

/* _explain_lstm_single_word_sequence(t) (E:537-666 / E:1180-1321) for n
 * (image, t) pairs at once.  img_idx_host[i] in [0,B), t_host[i] in
 * [1, len(caption_i)] (LRP_ERR_RANGE otherwise).  Outputs (device):
 *   R_feat_dev  (n, L, D)  float32   == the (1,sqrtL,sqrtL,D) return value
 *   att_dev     (n, L)     float32   attention_t (may be NULL)
 *   r_words_dev (n, max_caption_len) float64, entry j = self.r_words[j] for
 *               j < t-1 (adaptive, normalised, first dropped, E:660-665) or
 *               j < t (grid-TD, E:1320); rest 0 (may be NULL) */
int lrp_decoder_explain(lrp_handle* h, int32_t n, const int32_t* img_idx_host,
                        const int32_t* t_host, int32_t variant, float* R_feat_dev,
                        float* att_dev, double* r_words_dev, void* stream);

/* _explain_CNN(X, R) == LRPSequentialPresetA.analyze([X, R]) (E:179-181,
 * AB:478-520) for n relevance maps at once; image i uses the caches of
 * img_idx_host[i] from the last lrp_encode_images.  R_feat_dev (n,L,D),
 * R_img_dev (n,img_h,img_w,3) float32. */
int lrp_cnn_explain(lrp_handle* h, int32_t n, const int32_t* img_idx_host,
                    const float* R_feat_dev, float* R_img_dev, void* stream);

/* Fused a7->a10 chain for a batch: decoder explain + CNN explain without the
 * R_feat round trip through the caller (R_feat_dev / att_dev / r_words_dev may
 * be NULL when not wanted). */
int lrp_explain_tokens(lrp_handle* h, int32_t n, const int32_t* img_idx_host,
                       const int32_t* t_host, int32_t variant, float* R_img_dev,
                       float* R_feat_dev, float* att_dev, double* r_words_dev, void* stream);

/* ---- caption generation: incremental decoding for the beam search of explainers.py:51-120.
 * The reference re-runs the whole captioner on every partial caption at every search step; here the hypotheses'
 * decoder state lives on the device and a search step is ONE decoder step for all of them.  The beam bookkeeping
 * (BatchNLargest, completion rule) stays with the caller.
 * lrp_decoder_gen_begin: B rows = image slots of the cached features (for a beam of k per image, cache every image's
 *   features k times with lrp_set_features); zeroes the state.  Invalidates a previous lrp_decoder_forward.
 * lrp_decoder_gen_step: step s = 0 feeds SOS; for s > 0 row r continues the hypothesis of row parent_host[r] with
 *   tokenizer id word_host[r] appended (parent and child must be rows of the same image: only the recurrent state is
 *   re-parented, a row keeps its image's features).  logits_dev (B, V) float64 = the model's un-normalised scores for position s
 *   (column k = tokenizer id k+1), i.e. row s of `caption_preds`. */
int lrp_decoder_gen_begin(lrp_handle* h, int32_t B, void* stream);
int lrp_decoder_gen_step(lrp_handle* h, int32_t B, const int32_t* parent_host, const int32_t* word_host, int32_t step,
                         double* logits_dev, void* stream);
/* ABI v3.  The ranking step of the search on the device: `_log_softmax` (explainers.py:45-48) followed by
 * `np.argpartition(preds, -beam_size)[:, -beam_size:]` (explainers.py:76-78; inference.py:205-214) for `rows` rows of
 * un-normalised scores — only k (id, log p) pairs per hypothesis cross PCIe per search step, not the (beams, V) logits.
 * logits_dev (rows, V) float64; ids_dev (rows, k) int32 = model columns (tokenizer id - 1) by descending probability,
 * ties to the lower column; logp_dev (rows, k) float64.  1 <= k <= min(V, 32). */
int lrp_op_log_softmax_topk(const double* logits_dev, int32_t rows, int32_t V, int32_t k, int32_t* ids_dev,
                            double* logp_dev, void* stream);
/* The whole search on the device (added without raising the ABI version: nothing existing changed).  The bookkeeping of
 * explainers.py:51-120 — the two bounded heaps of `Caption(log_prob, sentence)` tuples (inference.py:267-315), the completion
 * rule, the final pick — as two kernels (csrc/beam_kernels.h): totals in float64, the k largest under the total order
 * (log_prob, sentence) by a counting rank, bit-identical to the host bookkeeping on the same scores.
 * lrp_decoder_beam_search: after lrp_decoder_gen_begin(h, n_images * k) on features laid out one slot per (image, beam).
 *   Enqueues `steps` iterations (re-parent, append, decoder step, logits, ranking, selection) and the finish on the stream:
 *   no host synchronisation and no copy.  Outputs (device): captions_dev (n_images, k, max_caption_len + 1) int32 tokenizer
 *   ids, zero-padded, every caption with a trailing EOS — the complete ones by descending order, then the live ones; row 0 is
 *   the reference's answer; lengths_dev (n_images, k) EOS included; logp_dev (n_images, k) float64; n_complete_dev (n_images).
 *   Refused before anything is launched: n_images * k > max_images, k outside [1, min(V, 32)], eos outside [1, V], rows other
 *   than the search was begun with (LRP_ERR_INVALID); steps outside [1, max_caption_len] (LRP_ERR_RANGE); no search begun
 *   (LRP_ERR_STATE).  Leaves the handle as lrp_decoder_gen_begin does: explain calls need a new lrp_decoder_forward.
 * lrp_op_beam_select / lrp_op_beam_finish: the same two kernels on caller-owned device buffers.  state_dev holds
 *   lrp_op_beam_state_bytes(n_images, k, max_len) bytes (8-byte aligned; a negative value for arguments the operators refuse)
 *   and needs no initialisation: step 0 starts a search.  Step s reads ids_dev / logp_dev (n_images * k, k) as
 *   lrp_op_log_softmax_topk writes them (at s = 0 only row 0 of an image is live) and writes parent_dev / word_dev
 *   (n_images * k): row r of step s + 1 continues row parent_dev[r] with tokenizer id word_dev[r].  Steps run in order
 *   0 .. steps - 1 <= max_len - 1, then lrp_op_beam_finish(steps) writes the outputs above with max_len in place of
 *   max_caption_len. */
int lrp_decoder_beam_search(lrp_handle* h, int32_t n_images, int32_t k, int32_t steps, int32_t eos, int32_t* captions_dev,
                            int32_t* lengths_dev, double* logp_dev, int32_t* n_complete_dev, void* stream);
int64_t lrp_op_beam_state_bytes(int32_t n_images, int32_t k, int32_t max_len);
int lrp_op_beam_select(void* state_dev, const int32_t* ids_dev, const double* logp_dev, int32_t n_images, int32_t k,
                       int32_t max_len, int32_t step, int32_t eos, int32_t* parent_dev, int32_t* word_dev, void* stream);
int lrp_op_beam_finish(const void* state_dev, int32_t n_images, int32_t k, int32_t max_len, int32_t steps, int32_t eos,
                       int32_t* captions_dev, int32_t* lengths_dev, double* logp_dev, int32_t* n_complete_dev, void* stream);

/* ---- gradient baselines on the same caches -------------------------------------------------
 * lrp_decoder_gradient == ExplainImgCaptioning{AdaptiveAttention,GridTD}Gradient._lstm_decoder_backward(t)
 * (models/explainers.py:780-832, :1452-1532) for n (image, t) units at once: d_feat_dev (n, L, D) float32 =
 * the reference's hand-written BPTT of logit[caption[t-1]-1] w.r.t. the CNN features (its simplifications
 * included); r_words_dev (n, max_caption_len) float64 or NULL, columns >= t untouched zeros.
 * Errors as lrp_decoder_explain, and LRP_ERR_UNSUPPORTED (before anything is allocated or launched) when
 *   - the decoder is LRP_DEC_ADAPTIVE and E != H: the reference's adaptive gradient class cannot run there
 *     (explainers.py:798 sizes d_xt E + H wide, :823 stores a 2E-wide row into it: ValueError), so no reference
 *     defines the result.  The grid-TD class runs at any E % 4 == 0 (goldens gridtd_grad_small_e16 / _e56 / _e20);
 *   - H, E or D is not a multiple of 4. */
int lrp_decoder_gradient(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const int32_t* t_host,
                         float* d_feat_dev, double* r_words_dev, void* stream);
/* lrp_cnn_walk == <Analyzer>(image_model, neuron_selection_mode="replace").analyze([X, head]) for
 * Gradient / InputTimesGradient / GuidedBackprop (innvestigate/analyzer/gradient_based.py:101-265;
 * explainers.py:672, :884, :928) — and LRPSequentialPresetA for LRP_WALK_LRP (same as lrp_cnn_explain).
 * head_dev (n, L, D) -> out_dev (n, img_h, img_w, 3).  Both encoders.  VGG-style encoders: every precision mode (the
 * gradient walks are exact fp32 in each).  ResNet encoder: the gradient walks run in LRP_PREC_FP32 only — its ReLU
 * decisions are recorded by the fp32-mode forward of lrp_encode_images, the other modes' forward keeps the inner
 * activations as fp16 pairs only — and return LRP_ERR_UNSUPPORTED in the other modes (set LRP_PREC_FP32 with
 * lrp_set_precision and call lrp_encode_images again); LRP_WALK_LRP runs in every mode.  The first gradient walk on a
 * ResNet handle after its weights changed packs a BN-scaled copy of the conv weights (counted in lrp_workspace_bytes,
 * like the ReLU masks the first fp32-mode encode allocates).
 * LRP_WALK_DECONVNET (gradient_based.py:180-225, DeconvnetReverseReLULayer): a layer with a ReLU clamps what arrives at 0 and
 * applies the gradient of the layer WITHOUT its activation; pools, BatchNorm, Add and padding take the plain gradient, pools
 * routing to the forward's arg-max (first in scan order on ties — an all-zero window included, whose share lands on its first
 * cell; in the ResNet stem that may be a padding cell, and the share is cropped away).  No forward ReLU decision is read, so
 * the walk runs in every precision mode on both encoders, in exact fp32.  Its first call after an encode builds a 0/1
 * position gate per pooled layer of a VGG-style encoder (max_images x that layer's activations, float32, allocated by the
 * first call and counted in lrp_workspace_bytes); the ResNet form allocates the BN-scaled matrices of the other gradient
 * walks and nothing else.
 * LRP_WALK_DEEPLIFT (added without a version bump; innvestigate/analyzer/deeplift.py:44-250, see lrp_set_deeplift_reference):
 * VGG-style handles in LRP_PREC_FP32 only.  LRP_ERR_UNSUPPORTED on a ResNet handle and in every other precision mode;
 * LRP_ERR_STATE without a reference, or when lrp_encode_images has not run since the reference was set or changed.
 * LRP_WALK_PATTERNNET / LRP_WALK_PATTERN_ATTRIBUTION (added without a version bump; analyzer/pattern_based.py:68-281, see
 * lrp_pattern_fit_begin): VGG-style handles in LRP_PREC_FP32 only, on the patterns the handle holds.  LRP_ERR_UNSUPPORTED on a
 * ResNet handle and in every other precision mode; LRP_ERR_STATE while a conv has no pattern, or with no encode. */
enum { LRP_WALK_LRP = 0, LRP_WALK_GRADIENT = 1, LRP_WALK_INPUT_X_GRADIENT = 2, LRP_WALK_GUIDED_BACKPROP = 3, LRP_WALK_DECONVNET = 4,
       LRP_WALK_DEEPLIFT = 5, LRP_WALK_PATTERNNET = 6, LRP_WALK_PATTERN_ATTRIBUTION = 7 };
int lrp_cnn_walk(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const float* head_dev, float* out_dev,
                 int32_t walk, void* stream);

/* Arithmetic of the per-token reverse walk through the encoder (lrp_cnn_explain / lrp_explain_tokens).
 * LRP_PREC_BF16X3 DEFAULT.  Split-bf16 walk: every fp32 operand is carried as hi + lo bf16 (16 mantissa bits) and every
 *                 product is hi*hi' + hi*lo' + lo*hi' on v_mfma_f32_32x32x16_bf16 with fp32 accumulation — three MFMAs
 *                 in every layer, no scaling state.  Worst case per product 2^-16 (8e-6 << the 1e-4 relative-L1 bar)
 *                 whatever the weights look like; measured 3e-6 ... 7e-6 on dense Gaussian and on sparse heavy-tailed
 *                 (trained-like) kernels alike (tests/test_gpu_stress_parity.py).  The per-image forward's activations
 *                 are fp32-grade (fp16 pairs on both operands, three MFMAs, blocked accumulation: 7e-7 on the features
 *                 like the fp32 MFMA); the denominators Z+ are three-term as well.
 * LRP_PREC_FP32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere: the reference's own arithmetic (TF float32).
 * LRP_PREC_F16X2  OPT-IN fast mode (VGG-style encoders; ABI v3).  The relevance tensors are fp16 pairs hi + lo carried
 *                 scaled by a per-token power of two; layers after the last pool take the full three-MFMA product, every
 *                 layer below with >= 64 output channels reads only the hi half of the weights: ONE fp16 (11 bits) per
 *                 weight, TWO MFMAs per product, and the denominators Z+ of those layers are computed with the same
 *                 rounded weights.  ~12 % faster than the default — but the weight rounding is the same for every token
 *                 and only averages out when a sum has many comparable products: 3-5e-6 on dense Gaussian kernels,
 *                 1e-4 ... 5e-4 (OUTSIDE the bar) on sparse heavy-tailed ones.  Worst case 2^-12 = 2.4e-4 per product.
 *                 Use it only after checking it on the model at hand (bench.py reports it as `fast_mode` with its own
 *                 in-run parity).  Conv widths % 8 != 0 silently use the fp32 path; the ResNet walk runs as BF16X3.
 * LRP_PREC_BF16X3_FAST  LRP_PREC_BF16X3 with two-way split activation convs in the forward as well: faster encode, but
 *                 arg-max flips put the heat-map parity at 2e-5 ... 9e-5 (five seeds).  Opt-in, not recommended.
 * The decoder is fp32 / fp64 in every mode.  A mode CHANGE drops the encode caches (the gates were computed in the old
 * arithmetic): lrp_encode_images must run again before the next explain call (LRP_ERR_STATE otherwise). */
enum { LRP_PREC_FP32 = 0, LRP_PREC_BF16X3 = 1, LRP_PREC_BF16X3_FAST = 2, LRP_PREC_F16X2 = 3 };
int lrp_set_precision(lrp_handle* h, int32_t mode);
/* ABI v5.  Which conv layers take the two-MFMA form in LRP_PREC_F16X2 mode: bit li of `mask` = the reverse launch through
 * conv li (and the forward denominators Z+ of that layer, which always follow it) reads ONE fp16 per weight; every other
 * layer takes the three-MFMA product on fp16 pairs (22 mantissa bits on both operands — at least as exact as
 * LRP_PREC_BF16X3).  mask = -1 restores the built-in rule (all layers up to the last pool with >= 576 products per sum);
 * mask = 0 is "fp16 pairs, three MFMAs everywhere".  This is the hook for a per-MODEL decision: calibration.py measures,
 * on the caller's own weights and images, the heat-map error each layer's two-term form causes against the exact-fp32
 * mode and enables it only where the measured error leaves the requested margin below the 1e-4 bar (the rule's error
 * depends on the weight statistics: see LRP_PREC_F16X2 above).  Layer 0 (the image layer) has no two-term form
 * (LRP_ERR_INVALID), nor have bits beyond the configured convs.  A change drops the encode caches when the handle is in
 * LRP_PREC_F16X2 mode (LRP_ERR_STATE from explain calls until lrp_encode_images ran again). */
int lrp_set_fast_layers(lrp_handle* h, int64_t mask);

/* ABI v10 (added without a version bump: purely additive).  The conv rule of the encoder's LRP walk: AlphaBetaRule (relevance_rule.py:216-322, bias = True) with
 * alpha >= 1, beta >= 0, alpha - beta == 1 (relevance_based/utils.py:72-129; anything else LRP_ERR_INVALID).  The two floats are
 * the caller's numbers rounded one by one, so the difference is checked to that rounding (|alpha - beta - 1| <= 6e-8 (alpha + beta):
 * (1.3f, 0.3f) is accepted, (2, 0.5) is not) and the walk uses beta = alpha - 1 in float.  Default (1, 0):
 * LRPSequentialPresetA / LRPAlpha1Beta0, the walk every handle has always run — that path is unchanged to the bit.
 * beta > 0 (LRPAlpha2Beta1 / LRPSequentialPresetB at (2, 1)): R_in = alpha act - beta inh with a second denominator
 * Z_inh = conv(x+, w-) + conv(x-, w+) + b per layer.  lrp_encode_images then also computes the inhibitor gates (one more
 * denominator conv per layer, in the handle's arithmetic: exact fp32 or three-term split-bf16), and the walk carries two
 * relevance chains through ONE GEMM per layer over the concatenated matrix [alpha w+ ; -beta w-] with a dual-gate epilogue
 * (DESIGN.md 4.15).  Max-pools route by gradient as before.  Followed by lrp_cnn_explain, lrp_explain_tokens,
 * lrp_cnn_walk(LRP_WALK_LRP) and everything built on them; the gradient walks ignore it.
 * A CHANGE drops the encode caches like lrp_set_precision: explain calls return LRP_ERR_STATE until lrp_encode_images ran
 * again.  The first beta > 0 allocates the second gates, the two-chain buffers, the kept layer inputs and the packed matrices
 * (counted in lrp_workspace_bytes; idle again at beta = 0); a handle that never sets a beta > 0 allocates nothing.
 * On a VGG-style handle the rule is the table of lrp_set_cnn_rules with this record, bias 1, on every conv: one rule state, and
 * the buffers are the table's (a later table that needs the same ones finds them there).
 * A ResNet handle takes the rule as well: per conv + BN unit a second gate with Z_inh = conv(x, w-) + b, computed by
 * lrp_encode_images behind the unchanged forward (the pair-emitting path: the unit's own launch again against [w | w-]), the walk
 * with units 3 and 2 of a bottleneck block as dual-gate launches and unit 1 / the projection as one-gate launches over both chains;
 * LRP_PREC_BF16X3 and LRP_PREC_FP32.  It needs a stem width and stack widths that are multiples of 8 (the dual gate's granularity).
 * LRP_ERR_UNSUPPORTED: beta > 0 on a ResNet handle with another width (at this call); from the explain calls with beta > 0 in
 * LRP_PREC_F16X2 (VGG-style encoders) or for a launch lrp_conv_plan refuses. */
int lrp_set_cnn_rule(lrp_handle* h, float alpha, float beta);

/* Added without a version bump (purely additive).  A rule per conv for the VGG-style encoder's LRP walk: the
 * relevance-rule half of LRP(model, rule=..., input_layer_rule=...), relevance_analyzer.py:343-415.  `rules` holds one record per
 * configured conv, input layer first; n_rules must equal the handle's number of convs.
 *   LRP_RULE_ALPHA_BETA  alpha, beta as lrp_set_cnn_rule checks them; bias 1 = AlphaBetaRule, 0 = AlphaBetaIgnoreBiasRule
 *                        (both denominators without the bias).  Any layer.
 *   LRP_RULE_EPSILON     eps >= 0; eps = 0 is ZRule (SafeDivide, no stabiliser), eps > 0 EpsilonRule: Z + (2 [Z >= 0] - 1) eps and a
 *                        plain divide; bias 1 / 0 = with / IgnoreBias.  Any layer; LRP_PREC_FP32 only.
 *   LRP_RULE_FLAT, LRP_RULE_WSQUARE   FlatRule / WSquareRule: Z = conv(1, 1) resp. conv(1, w^2) with 'same' padding (so it varies at
 *                        the border), no bias, R_in = convT(R / Z, 1 resp. w^2).  Layer 0 only.
 *   LRP_RULE_BOUNDED     BoundedRule with the scalars low < high.  Layer 0 only.
 * Fields a kind does not use are ignored.  LRP_ERR_INVALID: a wrong count, an unknown kind, bias outside {0, 1}, flat / w-square /
 * bounded above layer 0, eps < 0, low >= high, alpha / beta outside lrp_set_cnn_rule's check.  LRP_ERR_UNSUPPORTED: a ResNet handle;
 * an input-layer kind on a one-conv encoder.
 * lrp_set_cnn_rule(alpha, beta) IS the table with the same alpha-beta record with bias on every layer: the two entries set one rule
 * state and run the same code, to the bit ((1, 0) everywhere is the default walk, from either entry; the rule already set, from
 * either entry, changes and drops nothing), and lrp_set_cnn_rule in turn replaces any table.  Every other table runs the
 * dense table walk: layer l reads one or two relevance chains (two for alpha-beta with beta > 0) against one matrix and applies
 * layer l-1's one or two gates; lrp_encode_images adds the denominator passes the rules need behind the unchanged forward.
 * Alpha-beta kinds and the three input-layer kinds run in exact fp32 and in three-term split-bf16 with the handle; with an epsilon
 * kind in the table the explain calls return LRP_ERR_UNSUPPORTED outside LRP_PREC_FP32, and in LRP_PREC_F16X2 for every table.
 * LRP_ERR_UNSUPPORTED from the explain calls as well for a table with a launch lrp_conv_plan refuses: a one-chain layer on a
 * two-chain layer takes LRP_PLAN_DUAL_MUL with Cin(plan) = its width, a multiple of 16 (split-bf16) / 8 (fp32).  A CHANGE drops the encode caches (LRP_ERR_STATE from explain calls until lrp_encode_images ran
 * again).  Buffers appear with the first table that needs them, sized by that table's chain counts (a table that reads one chain
 * everywhere walks on the default walk's buffers), are counted in lrp_workspace_bytes and idle afterwards; a handle that never sets
 * a table allocates nothing. */
enum { LRP_RULE_ALPHA_BETA = 0, LRP_RULE_EPSILON = 1, LRP_RULE_FLAT = 2, LRP_RULE_WSQUARE = 3, LRP_RULE_BOUNDED = 4 };
typedef struct lrp_conv_rule {
  int32_t kind;        /* LRP_RULE_* */
  int32_t bias;        /* alpha-beta and epsilon kinds: 1 = the bias is a constant input, 0 = IgnoreBias */
  float alpha, beta;   /* LRP_RULE_ALPHA_BETA */
  float eps;           /* LRP_RULE_EPSILON */
  float low, high;     /* LRP_RULE_BOUNDED */
} lrp_conv_rule;
int lrp_set_cnn_rules(lrp_handle* h, const lrp_conv_rule* rules, int32_t n_rules);

/* Added without a version bump (purely additive).  The rule PAIR of a ResNet handle's LRP walk: `stem` for the
 * 7x7 stem conv (the input layer), `units` for every conv above it; BatchNorm, Add, the pad and the stem pool are reversed as
 * before whatever the pair.  Records as lrp_set_cnn_rules reads them:
 *   units  LRP_RULE_ALPHA_BETA (bias 1 or 0) or LRP_RULE_EPSILON (bias 1 or 0; eps = 0 is ZRule)
 *   stem   those, and LRP_RULE_FLAT, LRP_RULE_WSQUARE, LRP_RULE_BOUNDED.  The stem is a valid conv over the explicitly padded
 *          image, so all 147 taps count at every output pixel (flat: Z = 147; w-square: the sum of w^2 per channel; bounded: pad
 *          cells hold low / high like every other cell) and relevance sent to pad cells is cropped away.
 * The two records are independent: every combination runs.  lrp_set_cnn_rule(alpha, beta) IS the pair with that alpha-beta-with-
 * bias record twice: one rule state, the same code, to the bit; the pair already set changes and drops nothing.  Any other
 * change drops the encode caches (LRP_ERR_STATE from the explain calls until lrp_encode_images ran again).  Every other pair leaves
 * the forward as it is — the features are those of a handle that never set a rule, bit for bit — and lrp_encode_images makes the
 * pair's gates behind it with fp32 launches of the units' convs and one streaming kernel per gate.
 * LRP_ERR_INVALID: lrp_set_cnn_rules' value checks; an input-layer kind in `units`.  LRP_ERR_UNSUPPORTED: a VGG-style handle;
 * beta > 0 in either record on widths that are no multiples of 8 (as lrp_set_cnn_rule); from the explain calls for a pair with an
 * epsilon kind outside LRP_PREC_FP32, and for a launch lrp_conv_plan refuses.  Alpha-beta and the three input kinds run in
 * LRP_PREC_BF16X3 and LRP_PREC_FP32.  Buffers and matrices appear with the first pair that needs them, are counted in
 * lrp_workspace_bytes and idle afterwards; a handle that never sets a pair allocates nothing.  The gradient walks ignore the pair.
 * lrp_set_cnn_rules keeps answering LRP_ERR_UNSUPPORTED on a ResNet handle: a rule per conv of the branched graph is not built. */
int lrp_set_resnet_rules(lrp_handle* h, const lrp_conv_rule* stem, const lrp_conv_rule* units);

/* Added without a version bump (purely additive).  DeepLIFT on a VGG-style handle:
 *   DeepLIFT(model, neuron_selection_mode="replace", reference_inputs=r, approximate_gradient=...).analyze([X, head])
 * of innvestigate/analyzer/deeplift.py, where every Conv2D(activation='relu') takes LinearRule on the fused layer:
 *   t = dX * convT(M A / safe(dY)),  g = convT(M A),  out = |dX| < 1e-7 ? g : t   (approximate_gradient=False: out = t)
 * with dX = X - Xr, dY = Y - Yr against the forward of ONE reference shared by all images, safe(d) = d + 1e-7 [d == 0], M the ReLU
 * mask of the image's forward; max-pools take the plain gradient (the image's arg-max, first in scan order on ties); the head is
 * the caller's tensor.  ref_host: (img_h, img_w, 3) float32, or NULL for the constant ref_scalar.
 * mode 0 = off, 1 = approximate_gradient=False (one chain), 2 = True (two chains and the per-element select).
 * A change of reference or mode drops the encode caches, as lrp_set_cnn_rules does; the same setting again does nothing.  The
 * next lrp_encode_images in LRP_PREC_FP32 runs the reference through the images' own forward path as a batch of one (again only
 * after a weight, precision or reference change) and writes one gate per layer and image behind the unchanged forward; in the
 * other precision modes nothing is computed and LRP_WALK_DEEPLIFT answers LRP_ERR_UNSUPPORTED.  The LRP and gradient walks, the
 * features and the fine-tune step are, bit for bit, those of a handle without a reference.  Buffers appear with the first
 * mode != 0 (mode 2 adds the two-chain ping-pong of 2 max_tokens rows), are counted in lrp_workspace_bytes and idle afterwards;
 * a handle that never sets a reference allocates nothing.  LRP_ERR_UNSUPPORTED: a ResNet handle (its stand-alone Activation,
 * BatchNorm and Add layers take other mappings), or a launch lrp_conv_plan refuses.  LRP_ERR_INVALID: mode, a non-finite value. */
int lrp_set_deeplift_reference(lrp_handle* h, const float* ref_host, float ref_scalar, int32_t mode);

/* Layer trace (added without a version bump; innvestigate/analyzer/base.py:570-603, :715-802 — reverse_keep_tensors,
 * reverse_check_min_max_values, reverse_check_finite): the LRP walk of a VGG-style handle with the relevance at the input of every
 * layer materialised and reduced on the device.  The encoder's nodes are its convs and 2x2 max-pools in execution order,
 * nid = 0 .. N-1; the traced tensors, in sorted-id order, are index 0 = (-1, 0), the head as the caller passed it, and index
 * 1 + nid = (nid, 0), the relevance at the INPUT of node nid in that tensor's shape — index 1 is the image-level result.  A pool's
 * input tensor is at full resolution: the pool's output relevance at the forward's arg-max (first in scan order), exact 0.0
 * at the other three cells.  With LRP_MAX_CONV = 32 there are at most 64 tensors: every one has a bit in a 64-bit mask.
 * lrp_set_layer_trace: while on, the handle keeps every conv's input at encode (as a rule table does; counted in
 *   lrp_workspace_bytes).  A change drops the encode caches, as lrp_set_cnn_rules does; the same value again does nothing.
 *   Features, the other walks and the fine-tune step are, bit for bit, those of a handle that never saw the switch.
 * lrp_trace_tensor_count: N + 1.  lrp_trace_tensor_info: node id and shape of tensor `index`, and for a call with n rows and
 *   keep_mask (bit t = tensor index t) its offset in the keep buffer in floats (-1: not selected) and the buffer's size.
 * lrp_cnn_explain_traced: n heads (n, L, D) and img_idx_host as lrp_cnn_explain, under the rule in force (the default,
 *   lrp_set_cnn_rule or any lrp_set_cnn_rules table, one chain or two) in LRP_PREC_FP32 and LRP_PREC_BF16X3[_FAST].  Writes
 *   R_img_dev (n, img_h, img_w, 3); stats_dev (N + 1, n, 4) float64 — minimum, maximum, sum and count of non-finite elements of
 *   every traced tensor per row, from the fp32 values the keep buffer would hold (min / max exact, NaN where the row holds a
 *   NaN, -0.0 below +0.0; the sum accumulated in float64; reductions in a fixed order that depends neither on n nor on the
 *   other rows: a row's statistics and kept tensors are the same bits at n = 1 and inside a larger call); and, keep_dev not
 *   NULL, each tensor of keep_mask as (n, H, W, C) float32 at its offset.  Per layer it runs the rule's transposed conv with
 *   a plain fp32 accumulator and one streaming kernel (csrc/trace_kernels.h); its reduction partials are allocated by the first
 *   traced call (counted in lrp_workspace_bytes).
 *   LRP_ERR_UNSUPPORTED: a ResNet handle, LRP_PREC_F16X2, an epsilon table outside LRP_PREC_FP32, a launch lrp_conv_plan refuses.
 *   LRP_ERR_STATE: the switch is off, or lrp_encode_images has not run since it was turned on.  LRP_ERR_INVALID: n, a mask
 *   naming no tensor, keep_floats below what lrp_trace_tensor_info reports — nothing is launched.
 * lrp_op_tensor_stats: the same four statistics of x_dev (rows, per_row) float32 into stats_dev (rows, 4) float64; one block
 *   per row, a fixed order. */
int lrp_set_layer_trace(lrp_handle* h, int32_t on);
int32_t lrp_trace_tensor_count(lrp_handle* h);
int lrp_trace_tensor_info(lrp_handle* h, int32_t index, int32_t n, uint64_t keep_mask, int32_t* nid, int32_t* H, int32_t* W, int32_t* C,
                          int64_t* offset, int64_t* keep_floats);
int lrp_cnn_explain_traced(lrp_handle* h, int32_t n, const int32_t* img_idx_host, const float* R_feat_dev, float* R_img_dev,
                           double* stats_dev, uint64_t keep_mask, float* keep_dev, int64_t keep_floats, void* stream);
int lrp_op_tensor_stats(const float* x_dev, int32_t rows, int64_t per_row, double* stats_dev, void* stream);

/* PatternNet / PatternAttribution (added without a version bump; innvestigate/tools/pattern.py:220-336 — the fit — and
 * analyzer/pattern_based.py:68-281 — the walk).  VGG-style handles, LRP_PREC_FP32.  Fit and walk are independent: the walk runs on
 * whatever patterns the handle holds, fitted or set.
 * The fit, per conv: X = the im2col rows of the layer input (K = 9 cin, zero padded), Y = X W (no bias, no activation), mask per
 *   position and channel = 1 (LINEAR), [Y + b > 0] (RELU_POSITIVE) or [Y + b <= 0] (RELU_NEGATIVE).  Over every position of every
 *   image accumulated, in float64 on the device: Sx[k][c] = sum X_k mask_c, Sxy[k][c] = sum X_k Y_c mask_c, cnt[c] = sum mask_c,
 *   Sy[c] = sum Y_c, P = positions.  The pattern is A = cov / safe(sum_k W[k][c] cov[k][c]) with cov = Sxy / safe(cnt) -
 *   Sx / safe(cnt) * Sy / P and safe(v) = v + [v == 0]; a channel that never satisfies the mask gets zeros.
 * lrp_pattern_fit_begin: allocates and zeroes the sums (counted in lrp_workspace_bytes, as everything the pattern entries
 *   allocate), makes the handle keep every conv's input at encode and drops the encode caches.
 * lrp_pattern_fit_batch: accumulates the images of the last lrp_encode_images; a second call for the same encode is LRP_ERR_STATE.
 * lrp_pattern_fit_end: computes the patterns from the sums and installs them; the fit is closed, its sums stay readable.
 * lrp_pattern_stats: conv's sums as one float64 array [Sx (9 cin cout, HWIO) | Sxy (the same) | cnt (cout) | Sy (cout) | P (1)];
 *   n_doubles must be that size.
 * lrp_set_patterns / lrp_get_patterns: one conv's pattern, (3, 3, cin, cout) float32 on the device.
 * lrp_set_pattern_projection: reverse_project_bottleneck_layers (default 1): every reversed tensor — the head, the tensor at every
 *   conv's input, the result — is divided per row by its absolute maximum (1 where that is 0) before it is used.
 * The walks: per conv the ReLU's gradient, then the conv's gradient with the kernel replaced by A (PATTERNNET) or A * W
 *   (PATTERN_ATTRIBUTION); pools route to the forward's arg-max.  A row's result is the same bits at n = 1 and inside a larger call.
 * LRP_ERR_UNSUPPORTED: a ResNet handle; outside LRP_PREC_FP32 (fit entries and walks); a launch lrp_conv_plan refuses.
 * LRP_ERR_STATE: fit_batch / fit_end without fit_begin, fit_batch without an encode since or twice for one, fit_end without a
 *   batch, stats before any fit, get without a pattern, a walk while a conv has no pattern or without an encode.
 * LRP_ERR_INVALID: a conv index or type out of range, a wrong size.  Nothing is launched on a refusal. */
enum { LRP_PATTERN_LINEAR = 0, LRP_PATTERN_RELU_POSITIVE = 1, LRP_PATTERN_RELU_NEGATIVE = 2 };
int lrp_pattern_fit_begin(lrp_handle* h, int32_t type);
int lrp_pattern_fit_batch(lrp_handle* h, void* stream);
int lrp_pattern_fit_end(lrp_handle* h, void* stream);
int lrp_pattern_stats(lrp_handle* h, int32_t conv, double* sums_dev, int64_t n_doubles, void* stream);
int lrp_set_patterns(lrp_handle* h, int32_t conv, const float* A_hwio_dev, void* stream);
int lrp_get_patterns(lrp_handle* h, int32_t conv, float* A_hwio_dev, void* stream);
int lrp_set_pattern_projection(lrp_handle* h, int32_t on);

/* Dominant-kernel timing for bench.py's roofline block: when enabled, HIP
 * events bracket every conv-LRP launch on the caller's stream; query returns
 * launches and summed milliseconds since the last reset (syncs the events). */
int lrp_profile_enable(lrp_handle* h, int32_t on);
int lrp_profile_query(lrp_handle* h, int64_t* n_launches, double* total_ms, double* total_flop);
/* Same, per launch: fills up to `cap` entries of ms_out / flop_out (in launch order) and
 * returns the count in *n_out; the records are consumed. */
int lrp_profile_records(lrp_handle* h, int32_t cap, double* ms_out, double* flop_out, int32_t* n_out);

/* Workspace bytes held by the handle. */
int64_t lrp_workspace_bytes(const lrp_handle* h);

/* Operator-level entry (unit tests of the dominant kernel): implicit-GEMM
 * 3x3 'same' (taps=9) or 1x1 (taps=1) convolution on NHWC float32 with the
 * fp32 MFMA path.  w_hwio_host: (3,3,Cin,Cout) or (1,1,Cin,Cout).
 * mode 0: out = relu(conv + bias); mode 1: out = conv + bias;
 * mode 2: out = convT(in, w) * aux   (LRP backward with gate `aux`, shape of out)
 * mode 3: like 2 with 2x nearest up-sampling of the conv result (pool routing).
 * mode | LRP_CONV_SPLIT_BF16 (modes 1..3, channels % 8 == 0): the same operator on the split-bf16
 * MFMA path the engine uses by default (three bf16 MFMAs per fp32 product); in/out stay float32.
 * mode | LRP_CONV_SPLIT_BF16 | LRP_CONV_WREG (mode 2, taps = 9, Cin % 128 == 0, otherwise LRP_ERR_UNSUPPORTED): the entry also makes
 * the fragment-major copy of the weights, so that a launch on the 128 x 128 resident-image tile takes the weights-in-registers
 * loop (LRP_FORM_BREG4).  Without the bit such a launch keeps the pipelined kernel. */
enum { LRP_CONV_SPLIT_BF16 = 0x100, LRP_CONV_WREG = 0x200 };
int lrp_op_conv(const float* in_dev, const float* w_hwio_host, const float* bias_host,
                const float* aux_dev, float* out_dev, int32_t NB, int32_t H, int32_t W,
                int32_t Cin, int32_t Cout, int32_t taps, int32_t mode, void* stream);

/* ABI v10 (added without a version bump: purely additive).  Operator-level entry of the two-chain launch of the alpha-beta walk (lrp_set_cnn_rule, beta > 0), all tensors plain
 * fp32 NHWC:  c = convT(sp, alpha w+) + convT(sn, -beta w-)  (3x3 'same', ONE GEMM with K = 2 x 9 x Cout),
 *   outp = c x gp,  outn = c x gn       with c repeated 2 x 2 (nearest) when pool != 0.
 * sp_dev, sn_dev (NB, H, W, Cout); w_hwio_host (3, 3, Cin, Cout); gp_dev, gn_dev, outp_dev, outn_dev (NB, H u, W u, Cin), u = 2
 * with pool.  split != 0: on the split-bf16 path (channels % 8 == 0), fp32 otherwise (channels % 4 == 0).  The launch takes the
 * form lrp_conv_plan answers for LRP_PLAN_DUAL_MUL with Cin(plan) = 2 Cout, N(plan) = Cin.  It is lrp_op_conv_rule with
 * chains_in = gates_out = 2 and (p0, q0, p1, q1) = (alpha, 0, 0, -beta). */
int lrp_op_conv_ab(const float* sp_dev, const float* sn_dev, const float* w_hwio_host, float alpha, float beta, const float* gp_dev,
                   const float* gn_dev, float* outp_dev, float* outn_dev, int32_t NB, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                   int32_t pool, int32_t split, void* stream);

/* Added without a version bump (purely additive).  lrp_op_conv_ab for chains_in, gates_out in {1, 2} (the launches of the rule
 * table's walk, lrp_set_cnn_rules): chain j is multiplied with p_j w+ + q_j w-,
 *   c = sum_j convT(s_j, p_j w+ + q_j w-)   (3x3 'same', ONE GEMM with K = chains_in x 9 x Cout),   out_i = c x g_i,
 * c repeated 2 x 2 (nearest) when pool != 0.  s0_dev, s1_dev (NB, H, W, Cout); g_i / out_i (NB, H u, W u, Cin); s1_dev is not read
 * with one chain, g1_dev / out1_dev not with one gate.  split as in lrp_op_conv_ab.  Two gates take the form lrp_conv_plan answers
 * for LRP_PLAN_DUAL_MUL with Cin(plan) = chains_in x Cout, one gate the plain MUL epilogues' with the same Cin(plan); what the plan
 * refuses is LRP_ERR_UNSUPPORTED (one chain into two gates: Cout % 16 == 0 split, % 8 fp32). */
int lrp_op_conv_rule(const float* s0_dev, const float* s1_dev, const float* w_hwio_host, int32_t chains_in, int32_t gates_out, float p0,
                     float q0, float p1, float q1, const float* g0_dev, const float* g1_dev, float* out0_dev, float* out1_dev, int32_t NB,
                     int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pool, int32_t split, void* stream);

/* Added without a version bump (purely additive).  One fused conv + ReLU layer of the DeepLIFT walk as an operator, exact fp32,
 * all tensors plain fp32 NHWC.  With Y = relu(conv(x) + b), Yr = relu(conv(xr) + b), M = [Y > 0] (with pool != 0: and the first
 * arg-max of Y's 2x2 window, where a_dev, at pooled resolution, is routed to):
 *   out = mode 2 && |x - xr| < 1e-7 ? convT(M a) : (x - xr) * convT(M a / safe(Y - Yr))        (mode 1: always the second)
 * x_dev, out_dev (NB, H, W, Cin); xr_dev (H, W, Cin), shared by the batch; a_dev (NB, H u, W u, Cout), u = 1/2 with pool;
 * w_hwio_host (3, 3, Cin, Cout); bias_host (Cout).  Cout % 4 == 0; Cin % 4 == 0, or Cin == 3: the image layer's launches.
 * What lrp_conv_plan refuses is LRP_ERR_UNSUPPORTED. */
int lrp_op_deeplift_conv(const float* x_dev, const float* xr_dev, const float* a_dev, const float* w_hwio_host, const float* bias_host,
                         float* out_dev, int32_t NB, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t pool, int32_t mode, void* stream);

/* ABI v6.  The conv-LRP launch BEHIND a 2x2 max-pool (AlphaBetaRule RR:274-322 for a conv whose output feeds MaxPooling2D: the
 * relevance arrives through the pool's gradient routing, RA:470-480 -> IL:138-157, i.e. one non-zero per window and channel)
 * on the 2:4-sparse matrix cores (csrc/conv_sparse.h): out[n][y][x][ci] = gate[n][y][x][ci] x sum over taps, co of
 * S[n][y+dy][x+dx][co] w+[..], with S given in COMPACT form — sc_dev (NB, Hp, Wp, Cout) fp32 = the value of each window's
 * non-zero, pos_dev (same shape, bytes) = its position 2 dy + dx.  w_hwio_host (3, 3, Cin, Cout) like lrp_op_conv's backward
 * modes; gate_dev / out_dev (NB, 2 Hp, 2 Wp, Cin) fp32.  Split-bf16 arithmetic (three matrix instructions per product).
 * Needs Cin % 256 == 0, Cout % 16 == 0.  reps in 1 ... 255 repeats the launch (profiling); the bits above are not part
 * of this interface (the project's own measurement variants, SparseArgs::diag).  Same values as lrp_op_conv mode 2 with
 * LRP_CONV_SPLIT_BF16 on the expanded tensor up to the summation order (tests/test_gpu_conv_sparse.py). */
int lrp_op_conv_pool_sparse(const float* sc_dev, const unsigned char* pos_dev, const float* w_hwio_host, const float* gate_dev,
                            float* out_dev, int32_t NB, int32_t Hp, int32_t Wp, int32_t Cin, int32_t Cout, int32_t reps, void* stream);

/* Operator-level entries for the other rules LRPSequentialPresetA can reach (not on the
 * truncated-VGG16 path; ResNet-101 "next" row).  All pointers device memory unless `_host`.
 * EpsilonRule with bias=False (RR:113-144, RA:706-711): x (N,Din), W_host (Din,Dout) Keras
 * layout, R (N,Dout) -> out (N,Din).  Din, Dout multiples of 4. */
int lrp_op_epsilon_dense(const float* x_dev, const float* W_host, const float* R_dev, float* out_dev,
                         int32_t N, int32_t Din, int32_t Dout, float epsilon, void* stream);
/* BatchNormalizationReverseLayer (RA:197-257): channels-last x, R, out of n elements, C channels;
 * gamma/beta/mean/var device vectors of length C. */
int lrp_op_batchnorm_lrp(const float* x_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev,
                         const float* var_dev, float bn_eps, const float* R_dev, float* out_dev, int64_t n,
                         int32_t C, void* stream);
/* AddReverseLayer (RA:260-286): R_a = a*SafeDivide(R,a+b), R_b = b*SafeDivide(R,a+b). */
int lrp_op_add_lrp(const float* a_dev, const float* b_dev, const float* R_dev, float* Ra_dev, float* Rb_dev,
                   int64_t n, void* stream);

/* AveragePoolingReverseLayer (RA:289-316) for k x k / stride k 'valid' average pooling, channels-last:
 * x (NB,H,W,C), R (NB,H/k,W/k,C) -> out (NB,H,W,C) = x * SafeDivide(R, avgpool(x))[window] / k^2.
 * (Not reachable from either encoder cut — VGG16 block5_conv3, ResNet conv5_block3_out — provided as an operator.) */
int lrp_op_avgpool_lrp(const float* x_dev, const float* R_dev, float* out_dev, int32_t NB, int32_t H, int32_t W,
                       int32_t C, int32_t k, void* stream);

/* Heat-map rendering of explain_image.py:55-60 (`heatmap(postprocess(relevance))`, innvestigate/examples/
 * utils_imagenet.py:31-33 -> utils/visualizations.py:87-125, :57-80): per heat-map sign-preserving gamma correction
 * (0.95 in the reference), channel sum, abs-max projection to 0..255 and a 256 x 3 colormap lookup (lut_dev, the
 * reference uses matplotlib's 'seismic').  R_img_dev (n, npix, C) -> rgb_dev (n, npix, 3) float32.  An all-zero map
 * (0/0 and an undefined NaN->int cast in the reference) renders as the mid-scale colour. */
int lrp_heatmap_render(const float* R_img_dev, const float* lut_dev, float* rgb_dev, int32_t n, int32_t npix, int32_t C,
                       float gamma, void* stream);

/* Image preprocessing (models/preprocessors.py:38-53, vgg16 / vgg19 / resnet101 = keras preprocess_input 'caffe'):
 * rgb_dev (NB, H0, W0, 3) decoded uint8 RGB -> out_dev (NB, H, W, 3) float32: nearest-neighbour resize as PIL does
 * for load_img(target_size=(H, W)), RGB -> BGR, minus the ImageNet means.  The result feeds lrp_encode_images. */
int lrp_preprocess_images(const uint8_t* rgb_dev, float* out_dev, int32_t NB, int32_t H0, int32_t W0, int32_t H,
                          int32_t W, void* stream);

/* Score reduction of the LRP-inference layer (models/model.py:1675-1686) for n heat-maps:
 * hp = mean over channels, hp /= max|hp|, then mode 0 = mean, 1 = mean(max(hp,0)), 2 = np.quantile(hp, 0.9).
 * R_img_dev (n, npix, C) float32, scores_dev (n) float64. */
int lrp_heatmap_scores(const float* R_img_dev, double* scores_dev, int32_t n, int32_t npix, int32_t C, int32_t mode,
                       void* stream);

/* ABI v7.  Bounding-box correctness evaluation (evaluate_bbox.py:59-86, :191-272, EvaluationBboxCOCO /
 * EvaluationBboxCOCOBaseline): handle-free operators, device pointers, no synchronisation.  Per workgroup fixed-order
 * reductions, so a map's or an entry's results do not depend on what else shares the launch.
 * lrp_eval_relevance_maps: R_img_dev (n, npix, C) float32 (fp64 = 0) or float64 (fp64 = 1) relevance -> maps_dev (n, npix)
 *   in the same dtype, bit-identical to the reference's numpy chain: BGR -> RGB flip, multiply by `sign` (+1 / -1; the
 *   shipped script uses -1), max(., 0), channel mean, x / absmax (all zeros when absmax == 0).
 * lrp_eval_expand_matrix: host only, no GPU.  M_host (g * upscale, g) float64 with pyramid_expand(A, upscale, sigma) =
 *   M A M^T (skimage.transform.pyramid_expand: bilinear resize with mirrored edges, then a Gaussian blur of radius
 *   int(4 sigma + 0.5) with scipy's 'reflect' boundary).  g <= 16, g * upscale <= 448.
 * lrp_eval_attention_maps: att_dev (n, g * g) float32, M_dev = that matrix on the device -> maps_dev (n, S, S) float64,
 *   S = g * upscale: M A M^T followed by project() (x / absmax, then (x + 1) / 2 if any value is negative).
 * lrp_eval_box_scores: maps_dev (n, h, w) float32 / float64, boxes_dev (nb, 5) int32 = (map, y0, y1, x0, x1) with
 *   0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w (rows [y0, y1), columns [x0, x1)), thr_dev (nb, K) float64 with K <= 16 ->
 *   scores_dev (nb, K) float64 = sum over the box of v [v > thr] / sum over the map of v [v > thr], 0 when the
 *   denominator is 0, capped at 1.  An entry outside these bounds is not read and scores NaN.  The reference's threshold
 *   carry-over between the boxes of one word is the caller's: it goes into the per-entry thresholds. */
int lrp_eval_relevance_maps(const void* R_img_dev, void* maps_dev, int32_t fp64, int32_t n, int32_t npix, int32_t C,
                            int32_t sign, void* stream);
int lrp_eval_expand_matrix(int32_t g, int32_t upscale, double sigma, double* M_host);
int lrp_eval_attention_maps(const float* att_dev, const double* M_dev, double* maps_dev, int32_t n, int32_t g,
                            int32_t upscale, void* stream);
int lrp_eval_box_scores(const void* maps_dev, int32_t fp64, int32_t n, int32_t h, int32_t w, const int32_t* boxes_dev,
                        const double* thr_dev, int32_t nb, int32_t K, double* scores_dev, void* stream);

/* ABI v9.  Grad-CAM on the device and the word examination (explainers.py:939-949 / :1643-1653 with the product of :934;
 * exaimin_word.py:95-102, :131-160, :488-489): handle-free operators like lrp_eval_*, device pointers, no synchronisation,
 * one workgroup per unit with fixed-order fp64 reductions.
 * lrp_op_gradcam: n (image, word) units.  feat_dev (B, L, D) float32 (what lrp_get_features returns), img_idx_dev (n) int32
 *   on the device, grads_dev (n, L, D) float32 (lrp_decoder_gradient), M_dev (S, g) float64 (lrp_eval_expand_matrix on the
 *   device), L = g * g, S = g * upscale.  Per unit in fp64: w_c = mean_l grads[l][c], A[l] = sum_c feat[img][l][c] w_c,
 *   cam = max(M A M^T, 0), cam /= max|cam| + 1e-6 -> cam_dev (n, S, S) float64 (a cam that is nowhere positive: exact zeros).
 *   gb_dev (n, S * S, C) float32 (lrp_cnn_walk with LRP_WALK_GUIDED_BACKPROP) and out_dev (n, S * S, C) float64 =
 *   (double)gb * cam, or NULL for both: the cam only.  g <= 16, S <= 448, D a multiple of 8 up to 4096, C <= 64.  A unit whose
 *   image index is outside [0, B) reads nothing and comes out as NaN.
 * lrp_exam_maps: R_img_dev (n, H, W, C) float32 (fp64 = 0) or float64 (fp64 = 1) -> per pixel the channel mean in flipped
 *   channel order in the input dtype (no sign, no rectification), pool = 0 none / 1 max / 2 ave over k x k blocks (k divides H
 *   and W; max exact, ave accumulated in fp64), x / absmax (zeros when absmax == 0; no (x + 1) / 2 branch), |x| if absval.
 *   maps_dev: (n, H, W) in the input dtype, or (n, H/k, W/k) float64 when pooled; means_dev (n) float64, the fixed-order
 *   fp64 mean of that map.  Either output may be NULL, not both. */
int lrp_op_gradcam(const float* feat_dev, const int32_t* img_idx_dev, const float* grads_dev, const double* M_dev,
                   const float* gb_dev, double* cam_dev, double* out_dev, int32_t n, int32_t B, int32_t g, int32_t upscale,
                   int32_t D, int32_t C, void* stream);
int lrp_exam_maps(const void* R_img_dev, int32_t fp64, int32_t n, int32_t H, int32_t W, int32_t C, int32_t pool, int32_t k,
                  int32_t absval, void* maps_dev, double* means_dev, void* stream);

/* Augment and reduce of the reference's wrappers (innvestigate/analyzer/wrapper.py:78-345: GaussianSmoother behind SmoothGrad,
 * PathIntegrator behind IntegratedGradients).  Handle-free operators like lrp_op_gradcam: device pointers, the caller's stream, no
 * synchronisation; additive to the ABI.  (csrc/augment_kernels.h)
 * The sample matrix is (B * n, per_image) in np.repeat order (wrapper.py:169): row r = b * n + s is sample s of image b.  Every
 * entry works on the rows [r0, r0 + count) of it: out_dev / maps_dev hold those count rows only (row r0 first), x_dev is the
 * (B, per_image) float32 input.  A row's values are a pure function of (r, i) and the arguments, so any cut into chunks gives
 * the same bits.  B * n < 2^31, per_image >= 1 (any value: a tail group writes fewer than four values).
 * lrp_op_augment_gaussian: out[r][i] = x[b][i] + sigma * N(seed, r, i) (two float32 roundings).  N is Philox4x32-10
 *   (multipliers 0xD2511F53 and 0xCD9E8D57, Weyl key increments 0x9E3779B9 and 0xBB67AE85; the Random123 known answers are in
 *   tests/test_gradient_family_ref.py) with key = (seed & 0xFFFFFFFF, seed >> 32) and counter = (g & 0xFFFFFFFF, g >> 32, r, 0),
 *   g = i / 4.  Its outputs x0..x3 become two Box-Muller pairs with u = ((x >> 8) + 0.5) 2^-24:
 *   z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1), (z2, z3) alike from (u2, u3); element i takes z[i % 4];
 *   |z| <= 5.89.  float32 with the precise logf / log1pf / sincospif on exactly representable arguments, no fast-math intrinsic.
 * lrp_op_augment_path: mode 0: out[r][i] = x + (s / n) (x - ref) — literally what the reference computes (wrapper.py:268-288,
 *   :317-337 with layers.py:513-522: it starts at x and moves AWAY from the reference; s / n excludes 1); mode 1: the published
 *   path ref + (s / n) (x - ref).  ref_dev (B, per_image) float32, or NULL for the scalar ref_scalar.  Each of s / n, x - ref,
 *   the product and the sum is rounded to float32 on its own, as numpy does.
 * lrp_op_reduce_mean, phase 0 (accumulate): acc_dev (B, per_image) float64 += sum over the chunk's rows of each image, in
 *   ascending s, of post(maps[r][i]); post 0 none, 1 |.|, 2 square (gradient_based.py:110-137 post-processes a sample, then the
 *   mean is taken).  One thread per element, no atomics; launches accumulate in stream order, so the sum does not depend on the
 *   chunking.  The caller zeroes acc_dev first.  out_dev, x_dev, ref_dev, ref_scalar, has_factor are not read.
 *   phase 1 (finish): out_dev (B, per_image) float32 = float(acc / n) or, has_factor = 1, float(acc / n * (x - ref)) with the
 *   product in float64 (wrapper.py:290-296, :339-345), rounded once.  maps_dev, r0, count, post are not read. */
int lrp_op_augment_gaussian(const float* x_dev, float* out_dev, int32_t B, int32_t n, int64_t per_image, int32_t r0, int32_t count,
                            float sigma, uint64_t seed, void* stream);
int lrp_op_augment_path(const float* x_dev, const float* ref_dev, float ref_scalar, float* out_dev, int32_t B, int32_t n,
                        int64_t per_image, int32_t r0, int32_t count, int32_t mode, void* stream);
int lrp_op_reduce_mean(int32_t phase, const float* maps_dev, double* acc_dev, int32_t B, int32_t n, int64_t per_image, int32_t r0,
                       int32_t count, int32_t post, float* out_dev, const float* x_dev, const float* ref_dev, float ref_scalar,
                       int32_t has_factor, void* stream);

/* ABI v10.  Perturbation ("pixel-flipping") analysis on the device (PT: = innvestigate/tools/perturbate.py): rank the regions
 * of a heat-map, replace the top-k regions of the image, read the explained word's score off the next forward.  Operators like
 * lrp_eval_* / lrp_exam_maps: device pointers, no synchronisation, one workgroup per unit with fixed-order fp64 reductions, so
 * a unit's result does not depend on what else shares the launch.  (csrc/perturb_kernels.h)
 * Geometry (PT:105-116, PT:170), shared by the first two entries: a map of H x W is cut into regions of rh x rw.  If rh divides
 *   H and rw divides W nothing is padded; if neither divides, each axis is padded by r - dim % r, floor(pad / 2) before and the
 *   rest after, in np.pad's 'reflect' mode (the edge sample is not repeated) — by index arithmetic, nothing padded is stored.
 *   If exactly one axis is divisible the reference pads it by a whole region and fails its assert at PT:107: LRP_ERR_INVALID.
 *   nreg = Hr * Wr regions in row-major order; more than 4096 regions, or a region side below 1: LRP_ERR_RANGE.
 * lrp_perturb_ranks (PT:167, PT:125-128, PT:79-84): R_img_dev (n, H, W, C) float32 (fp64 = 0) or float64 (fp64 = 1);
 *   reduce over the channels and aggregate over a region, each 0 = mean or 1 = max (np.mean / np.max).  Everything is
 *   accumulated in fp64 from the input dtype in one fixed order: a pixel is ((c0 + c1) + ...) / C, a region the sum of its
 *   pixels in raster order / (rh * rw); negate = 1 negates the score (least relevant first).  ranks_dev (n, nreg) int32:
 *   rank[i] = #{j : s_j > s_i or (s_j == s_i and j < i)}, 0 = the highest score; exact ties go to the lower region index (the
 *   reference sorts with quicksort and leaves their order open), NaN scores rank last.  scores_dev (n, nreg) float64 or NULL.
 * lrp_perturb_apply (PT:74-76, PT:130-148, PT:182-185): out_dev (n, H, W, C) float32: unit u is image img_idx_dev[u] of
 *   x_dev (B, H, W, C) float32 with every region of rank <= k_dev[u] - 1 replaced (k float64, as PT:385 adds a float
 *   regions_per_step).  mode 0 zeros, 1 mean (the fp64 raster-order mean of the padded region, reflected pixels included,
 *   per channel, rounded once to float32), 2 invert (-x), 3 noise (copies noise_dev (n, H, W, C) inside the perturbed regions:
 *   'gaussian' with the draw left to the caller; noise_dev is NULL for every other mode).  all_channels = 0 perturbs channel 0
 *   only, as the reference does (its mask has a channel axis of length 1 and PT:135-139 index x with that channel); 1 perturbs
 *   every channel.  has_range: np.clip to [lo, hi] (PT:142-146) of the whole unit, every channel, iff k >= 1 (one region is
 *   perturbed); the reference clips inside its loop, so what it perturbs afterwards is the clipped tensor: the unit is clipped,
 *   perturbed, and clipped again.  A unit whose image index is outside [0, B) reads nothing and comes out as NaN.
 * lrp_perturb_word_scores: the score of the explained word on the handle's cached forward (lrp_decoder_forward), read in
 *   place.  slot_dev, t_dev, k_dev (n) int32 on the device: image slot, position t >= 1, model column (token id - 1) ->
 *   logit_dev, logp_dev (n) float64: l[k] and l[k] - (max + log sum exp(l - max)) over row t - 1 of caption_preds.  A unit
 *   outside the cached logits reads nothing and comes out as NaN.  LRP_ERR_STATE without a forward. */
int lrp_perturb_ranks(const void* R_img_dev, int32_t fp64, int32_t n, int32_t H, int32_t W, int32_t C, int32_t rh, int32_t rw,
                      int32_t reduce, int32_t aggregate, int32_t negate, int32_t* ranks_dev, double* scores_dev, void* stream);
int lrp_perturb_apply(const float* x_dev, const int32_t* img_idx_dev, const int32_t* ranks_dev, const double* k_dev,
                      const float* noise_dev, float* out_dev, int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t rh,
                      int32_t rw, int32_t mode, int32_t all_channels, int32_t has_range, float lo, float hi, void* stream);
int lrp_perturb_word_scores(lrp_handle* h, const int32_t* slot_dev, const int32_t* t_dev, const int32_t* k_dev, int32_t n,
                            double* logit_dev, double* logp_dev, void* stream);

/* Occlusion sensitivity (Zeiler & Fergus 2014) and RISE (Petsiuk et al. 2018) word saliency: masked copies of the image go
 * through lrp_encode_images / lrp_decoder_forward / lrp_perturb_word_scores, and the word scores are folded back into a map.
 * Handle-free operators like lrp_op_augment_* and lrp_perturb_*: device pointers, the caller's stream, no synchronisation;
 * additive to the ABI.  Every argument is checked before any HIP call.  A row's output is a pure function of its arguments: any
 * cut of the rows into calls, and any position of a row in a call, gives the same bits.  (csrc/saliency_kernels.h)
 * Occlusion geometry: window (ph, pw), stride (sh, sw) with 1 <= sh <= ph <= H and 1 <= sw <= pw <= W (else LRP_ERR_INVALID);
 *   Hn = ceil((H - ph) / sh) + 1, Wn alike; window k = i * Wn + j covers rows [i sh, min(i sh + ph, H)) and columns
 *   [j sw, min(j sw + pw, W)): the last window of an axis is clipped, every pixel is covered.  More than 65536 windows:
 *   LRP_ERR_RANGE.
 * lrp_op_occlude: out_dev (n, H, W, C) float32: row r is image img_idx_dev[r] of x_dev (B, H, W, C) with window k_dev[r] set to
 *   fill_dev[c] (C floats on the device), every channel; k = -1 copies the image (the unoccluded score).  An image index outside
 *   [0, B) or a k outside [-1, Hn Wn) gives a NaN row.  16-byte accesses when H W C % 4 == 0 and both tensors are 16-byte aligned.
 * lrp_op_occlusion_map: scores_dev (n_img, 1 + Hn Wn, T) float64, row 0 the unoccluded score -> out_dev (n_img, T, H, W) float32:
 *   S[t][y][x] = (sum over the windows k covering (y, x), ascending k, of s_0[t] - s_{1+k}[t]) / c(y, x), c the number of covering
 *   windows, in float64, rounded once.  A gather: no atomics.
 * lrp_op_rise_grids: mask (key, k) -> grid_dev (n, (s + 1)^2) uint8 cells in {0, 1} and shift_dev (n, 2) int32 (dy, dx).  key_dev
 *   (n) uint32 is the caller's identity of the image, not its slot; k_dev (n) int32 the mask number.  Philox4x32-10 as in
 *   lrp_op_augment_gaussian with key = (seed & 0xFFFFFFFF, seed >> 32): cell e = a (s + 1) + c takes lane e % 4 of counter
 *   (e / 4, k, key, 1) (the last word 1 separates the stream from the Gaussian augment's 0); G = 1 iff (x >> 8) < floor(p 2^24)
 *   (computed in double; p = 1: all ones).  The shifts come from counter (0xFFFFFFFF, k, key, 1): dy = x0 % ch, dx = x1 % cw;
 *   the modulo bias (at most ch / 2^32) is accepted.  1 <= s <= 63 (else LRP_ERR_RANGE); 0 < p <= 1, ch >= ceil(H / s),
 *   cw >= ceil(W / s), ch, cw <= 2^20 (else LRP_ERR_INVALID).
 * lrp_op_rise_apply: out_dev (n, H, W, C) = fill + m (x - fill) in float32, each operation rounded on its own, row r from image
 *   img_idx_dev[r] with the mask of grid_dev[r], shift_dev[r].  The mask at pixel (y, x): Y = y + dy, ny = 2 Y + 1 - ch,
 *   a0 = floor_div(ny, 2 ch), fy = (ny - 2 ch a0) / (2 ch), rows a0 and a0 + 1 clamped into [0, s]; columns alike;
 *   m = top + fy (bot - top) with top = G[a0][c0] + fx (G[a0][c1] - G[a0][c0]) and bot alike on row a1: the half-pixel-centre
 *   bilinear upsample of the (s + 1)^2 grid by exactly (ch, cw), cropped at (dy, dx).  (RISE itself resizes an s x s grid by a
 *   non-integer factor; the two agree in distribution away from the border.)  A row whose image index is outside [0, B) or whose
 *   shift is outside [0, ch) x [0, cw) comes out as NaN.
 * lrp_op_rise_map: scores_dev (n_img, K, T) float64, grid_dev (n_img, K, (s + 1)^2), shift_dev (n_img, K, 2) -> out_dev
 *   (n_img, T, H, W) float32: S[t][y][x] = (sum over k ascending of s_k[t] m_k(y, x)) / (K p), masks recomputed in float64 from
 *   the grids, one thread per pixel adding its K terms in ascending k (the order depends on K only), rounded once. */
int lrp_op_occlude(const float* x_dev, const int32_t* img_idx_dev, const int32_t* k_dev, const float* fill_dev, float* out_dev,
                   int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ph, int32_t pw, int32_t sh, int32_t sw,
                   void* stream);
int lrp_op_occlusion_map(const double* scores_dev, float* out_dev, int32_t n_img, int32_t T, int32_t H, int32_t W, int32_t ph,
                         int32_t pw, int32_t sh, int32_t sw, void* stream);
int lrp_op_rise_grids(const uint32_t* key_dev, const int32_t* k_dev, int32_t n, int32_t s, double p, uint64_t seed, int32_t H,
                      int32_t W, int32_t ch, int32_t cw, uint8_t* grid_dev, int32_t* shift_dev, void* stream);
int lrp_op_rise_apply(const float* x_dev, const int32_t* img_idx_dev, const uint8_t* grid_dev, const int32_t* shift_dev,
                      const float* fill_dev, float* out_dev, int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s,
                      int32_t ch, int32_t cw, void* stream);
int lrp_op_rise_map(const double* scores_dev, const uint8_t* grid_dev, const int32_t* shift_dev, float* out_dev, int32_t n_img,
                    int32_t K, int32_t T, int32_t H, int32_t W, int32_t s, double p, int32_t ch, int32_t cw, void* stream);

/* The class-activation-map family as word saliencies: the gradient forms Grad-CAM (Selvaraju et al. 2017), Grad-CAM++
 * (Chattopadhay et al. 2018), XGrad-CAM (Fu et al. 2020), LayerCAM (Jiang et al. 2021) and HiResCAM (Draelos & Carin 2020), and
 * the gradient-free forms Score-CAM (Wang et al. 2020) and Ablation-CAM (Desai & Ramaswamy 2020), whose channel weights come from
 * forwards (lrp_encode_images or lrp_set_features, lrp_decoder_forward, lrp_perturb_word_scores).  Handle-free operators like
 * lrp_op_gradcam and lrp_op_rise_*: device pointers, the caller's stream, no synchronisation; additive to the ABI.  Every
 * argument is checked before any HIP call.  One workgroup per unit, (image, word) or slice of a row, fixed-order fp64
 * reductions, no float atomics: an output is a pure function of its own arguments, so any cut into calls and any neighbours
 * in a launch give the same bits.  (csrc/cam_kernels.h)
 * Shared: feat_dev (B, L, D) float32 (lrp_get_features), L = g * g, S = g * upscale, M_dev (S, g) float64
 *   (lrp_eval_expand_matrix on the device); g <= 16, S <= 448, D a multiple of 8 up to 4096.
 *   The finish, from a coarse map A (L) in fp64: cam = max(M A M^T, 0), cam /= max(cam) + 1e-6 (a cam that is nowhere positive:
 *   exact zeros) — the finish of lrp_op_gradcam, operation for operation.
 * lrp_op_cam: arguments as lrp_op_gradcam, plus mode.  Per unit u with F = feat[img_idx[u]] and G = grads[u], (L, D), in fp64:
 *   mode 0 gradcam    w_c = mean_l G[l][c];                                                    A[l] = sum_c F[l][c] w_c
 *   mode 1 gradcam++  S_c = sum_l F[l][c], den = 2 G^2 + S_c G^3, alpha = den != 0 ? G^2 / den : 0 (per l, c),
 *                     w_c = sum_l alpha[l][c] max(G[l][c], 0);                                 A[l] = sum_c F[l][c] w_c
 *   mode 2 xgradcam   w_c = sum_l F[l][c] G[l][c] / (sum_l F[l][c] + 1e-7);                    A[l] = sum_c F[l][c] w_c
 *   mode 3 layercam   A[l] = sum_c max(G[l][c], 0) F[l][c]
 *   mode 4 hirescam   A[l] = sum_c G[l][c] F[l][c]
 *   then the finish -> cam_dev (n, S, S) float64, and the optional gate out_dev (n, S * S, C) float64 = (double)gb * cam
 *   (gb_dev and out_dev both or neither; C <= 64), which generalises Guided Grad-CAM to every form.  Mode 0 equals
 *   lrp_op_gradcam bit for bit.  A unit whose image index is outside [0, B) reads nothing and comes out as NaN.
 * lrp_op_cam_weighted: scores_dev (n_img, R, T) float64: row 0 the unmasked image, row 1 + k channel k, and for mode 1 row
 *   1 + D the fill image; R = 1 + D (modes 0, 2) or 2 + D (mode 1), else LRP_ERR_INVALID.  img_idx_dev (n_img) int32: the image's
 *   row of feat_dev.  Per (image, word t), with s_k = scores[1 + k][t]:
 *   mode 0 softmax    w_k = exp(s_k - max_k s) / sum_k exp(s_k - max_k s), the sum in ascending k
 *   mode 1 linear     w_k = s_k - s_fill
 *   mode 2 ablation   w_k = (s_0 - s_k) / |s_0|; every weight 0 where s_0 == 0
 *   A[l] = sum_c F[l][c] w_c, then the finish -> cam_dev (n_img, T, S, S) float64 and / or map_dev (n_img, T, S, S) float32, the
 *   cam rounded once (either may be NULL, not both).  A NaN score makes that word's map NaN and nothing else; an image index
 *   outside [0, B) makes the image's maps NaN.
 * lrp_op_scorecam_apply: x_dev (B, H, W, C) float32 with H = W = g * upscale, k_dev (n) int32, fill_dev (C) float32 -> out_dev
 *   (n, H, W, C) float32.  Row r with k in [0, D): the channel map v[l] = feat[img][l][k] is min-max normalised on the g x g grid
 *   in float32, (v - min) / (max - min) with each operation rounded on its own (all zeros where max == min), then upsampled by
 *   exactly `upscale` pixels per cell with the half-pixel-centre bilinear rule of lrp_op_rise_apply at shift 0 (ny = 2 y + 1 -
 *   upscale, a0 = floor_div(ny, 2 upscale), fy = (ny - 2 upscale a0) / (2 upscale)), rows and columns clamped into [0, g - 1];
 *   out = fill + m (x - fill) in its float32 rounding order.  (Normalising before the upsample equals normalising after it: a
 *   bilinear interpolant takes its extremes at the nodes.)  k = -1 copies the image, k = D gives the fill image.  An image index
 *   outside [0, B) or a k outside [-1, D] gives a NaN row.  16-byte accesses when H W C % 4 == 0 and both tensors are 16-byte
 *   aligned.  n <= 65535 rows per call; D >= 1 (any value).
 * lrp_op_feature_ablate: out_dev (n, L, D) float32: row r is feat[img_idx_dev[r]] with channel k_dev[r] set to 0 (a copy
 *   otherwise: bit-exact); k = -1 copies the features.  An image index outside [0, B) or a k outside [-1, D) gives a NaN row.
 *   Any L, D >= 1. */
#define LRP_CAM_GRADCAM 0
#define LRP_CAM_GRADCAMPP 1
#define LRP_CAM_XGRADCAM 2
#define LRP_CAM_LAYERCAM 3
#define LRP_CAM_HIRESCAM 4
#define LRP_CAMW_SOFTMAX 0
#define LRP_CAMW_LINEAR 1
#define LRP_CAMW_ABLATION 2
int lrp_op_cam(const float* feat_dev, const int32_t* img_idx_dev, const float* grads_dev, const double* M_dev, const float* gb_dev,
               double* cam_dev, double* out_dev, int32_t n, int32_t B, int32_t g, int32_t upscale, int32_t D, int32_t C,
               int32_t mode, void* stream);
int lrp_op_cam_weighted(const double* scores_dev, const float* feat_dev, const int32_t* img_idx_dev, const double* M_dev,
                        double* cam_dev, float* map_dev, int32_t n_img, int32_t R, int32_t T, int32_t B, int32_t g, int32_t upscale,
                        int32_t D, int32_t mode, void* stream);
int lrp_op_scorecam_apply(const float* x_dev, const float* feat_dev, const int32_t* img_idx_dev, const int32_t* k_dev,
                          const float* fill_dev, float* out_dev, int32_t n, int32_t B, int32_t g, int32_t upscale, int32_t C,
                          int32_t D, void* stream);
int lrp_op_feature_ablate(const float* feat_dev, const int32_t* img_idx_dev, const int32_t* k_dev, float* out_dev, int32_t n,
                          int32_t B, int32_t L, int32_t D, void* stream);

/* LIME (Ribeiro et al. 2016) and KernelSHAP (Lundberg & Lee 2017) word saliency: the mask is a binary choice over d segments of
 * the image (label_dev: an int32 label map from any segmenter), the masked copies go through the same forwards as above and the
 * word scores are folded by a weighted linear regression.  Handle-free operators like lrp_op_rise_*: device pointers, the
 * caller's stream, no synchronisation; additive to the ABI.  Every argument is checked before any HIP call.
 * (csrc/segment_kernels.h)
 * Segments: 2 <= d <= 128 (else LRP_ERR_RANGE).  A row's subset is 4 uint32 words: bit j of word j / 32 is segment j, bits at or
 *   above d are zero.
 * lrp_op_segment_draws: row (key, k) -> bits_dev (n, 4) uint32.  key_dev (n) uint32 is the caller's identity of the image, k_dev
 *   (n) int32 the draw number.  Philox4x32-10 as in lrp_op_rise_grids with key = (seed & 0xFFFFFFFF, seed >> 32); the last
 *   counter word is 2 for LRP_SEGMENT_BERNOULLI and 3 for LRP_SEGMENT_SHAPLEY (0: the Gaussian augment, 1: RISE).
 *   Bernoulli (LIME): segment j takes lane j % 4 of counter (j / 4, k, key, 2), on iff (x >> 8) < floor(p 2^24); 0 < p <= 1.
 *   Shapley (KernelSHAP), pair q = k >> 1: u = lane 0 of counter (0xFFFFFFFF, q, key, 3); size s = 1 + #{i : u >= thr[i]} in
 *   [1, d - 1], thr_dev (d - 2) uint32 on the device (NULL allowed at d = 2 only): thr[i] = min(2^32 - 1, floor(C(i + 1) 2^32))
 *   with C the cumulative of p(m) ~ (d - 1) / (m (d - m)), m = 1 .. d - 1, computed by the caller in double.  Partial
 *   Fisher-Yates over perm = 0 .. d - 1: for i = 0 .. s - 1, r = lane i % 4 of counter (i / 4, q, key, 3),
 *   j = i + mulhi32(r, d - i), swap perm[i], perm[j]; the subset is perm[0 .. s).  An odd k is the complement within d bits of
 *   draw k - 1 (antithetic pairs).  p is not read in Shapley mode, thr_dev not in Bernoulli mode.  A row is a pure function of
 *   (seed, key, k, d, p or thr): any cut or order of the rows into calls gives the same bits.  An unknown mode, a p outside
 *   (0, 1] or a missing thr_dev: LRP_ERR_INVALID.
 * lrp_op_segment_apply: out_dev (n, H, W, C) float32: row r is image img_idx_dev[r] of x_dev (B, H, W, C) with every pixel whose
 *   segment label_dev[img][y][x] is off in bits_dev[r] set to fill_dev[c]: a select, no arithmetic, so all bits set reproduces
 *   the image.  An image index outside [0, B) gives a NaN row, a label outside [0, d) a NaN pixel.  16-byte accesses when
 *   H W C % 4 == 0 and both tensors are 16-byte aligned.
 * lrp_op_segment_fit: bits_dev (n_img, K, 4), wtab_dev (d + 1) float64, y_dev (n_img, K, T) float64 -> phi_dev (n_img, T, d),
 *   icpt_dev (n_img, T) float64, status_dev (n_img) int32.  Row weight w_k = wtab[popcount(z_k)]; weight 0 drops the row.
 *   delta_dev NULL (LIME form): minimise sum_k w_k (y_k - b - z_k . phi)^2 + ridge |phi|^2, b free and unpenalised (icpt = b).
 *   delta_dev (n_img, T) (Shapley form): phi_{d-1} = delta - sum_{j<d-1} phi_j, minimise sum_k w_k (y_k - z_{k,d-1} delta -
 *   sum_{j<d-1} (z_kj - z_{k,d-1}) phi_j)^2 + ridge sum_{j<d-1} phi_j^2: the efficiency constraint by elimination; icpt = 0.
 *   All in float64.  Every entry of the normal equations is a sum over k in ascending order, by one thread; the Gram matrix is
 *   shared by the T words of an image, each word its own right-hand side; Cholesky, one workgroup per image, the packed factor
 *   in LDS.  A pivot that is <= 0 or not finite sets status = 1 and the image's phi and icpt to NaN (else status = 0); a
 *   near-singular system is not detected.  An image's phi has the same bits at n_img = 1 and in any batch, a word's alone and
 *   among T others.  ridge < 0 or not finite: LRP_ERR_INVALID.
 * lrp_op_segment_map: phi_dev (n_img, T, d) float64, label_dev (n_img, H, W) int32 -> out_dev (n_img, T, H, W) float32:
 *   out = (float) phi[t][label], rounded once; a label outside [0, d) gives NaN. */
#define LRP_SEGMENT_BERNOULLI 0
#define LRP_SEGMENT_SHAPLEY 1
int lrp_op_segment_draws(const uint32_t* key_dev, const int32_t* k_dev, int32_t n, int32_t d, int32_t mode, double p,
                         const uint32_t* thr_dev, uint64_t seed, uint32_t* bits_dev, void* stream);
int lrp_op_segment_apply(const float* x_dev, const int32_t* img_idx_dev, const uint32_t* bits_dev, const int32_t* label_dev,
                         const float* fill_dev, float* out_dev, int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t d,
                         void* stream);
int lrp_op_segment_fit(const uint32_t* bits_dev, const double* wtab_dev, const double* y_dev, const double* delta_dev, double ridge,
                       double* phi_dev, double* icpt_dev, int32_t* status_dev, int32_t n_img, int32_t K, int32_t T, int32_t d,
                       void* stream);
int lrp_op_segment_map(const double* phi_dev, const int32_t* label_dev, float* out_dev, int32_t n_img, int32_t T, int32_t H,
                       int32_t W, int32_t d, void* stream);

/* Operator-level entries of the fine-tune step's dense products (unit tests at real layer sizes; csrc/train_gemm.h).
 * lrp_op_sgemm: C (+)= op(A) op(B) on the fp32 matrix cores, row-major with leading dimensions;
 *   op(A)[m][k] = transA ? A[k*lda + m] : A[m*lda + k], op(B)[k][n] = transB ? B[n*ldb + k] : B[k*ldb + n]
 *   (not both transposed).  ws_dev / ws_floats: scratch for the split over K (NULL: no split).
 * lrp_op_conv_wgrad: weight and bias gradient of a 3x3 'same' convolution: x (NB,H,W,Cin), dz (NB,H,W,Cout) ->
 *   dw (3,3,Cin,Cout) HWIO, db (Cout) or NULL; all nine taps in one launch, K = NB*H*W split deterministically. */
int lrp_op_sgemm(const float* A_dev, const float* B_dev, float* C_dev, int32_t M, int32_t N, int64_t K, int64_t lda, int64_t ldb,
                 int64_t ldc, int32_t transA, int32_t transB, int32_t accumulate, float* ws_dev, int64_t ws_floats, void* stream);
int lrp_op_conv_wgrad(const float* x_dev, const float* dz_dev, float* dw_hwio_dev, float* db_dev, int32_t NB, int32_t H, int32_t W,
                      int32_t Cin, int32_t Cout, float* ws_dev, int64_t ws_floats, void* stream);
/* the same product with bf16 operands (LRP_TRAIN_BF16; csrc/train_gemm_bf16.h) */
int lrp_op_conv_wgrad_bf16(const float* x_dev, const float* dz_dev, float* dw_hwio_dev, float* db_dev, int32_t NB, int32_t H,
                           int32_t W, int32_t Cin, int32_t Cout, float* ws_dev, int64_t ws_floats, void* stream);

/* ---- Fine-tune step of the LRP-inference training loop (train.py:573-581:
 * `keras_model.train_on_batch(X + [lrp_weight], [y, y])` on ImgCaptioningAdaptiveAttentionLRPInferenceModel,
 * models/model.py:1340-1374, and its grid-TD twin, train.py:645-656 on ImgCaptioningGridTDLRPInferenceModel,
 * models/model.py:1254-1311; VGG encoder, the decoder the handle was created with).  Per batch the caller runs lrp_encode_images,
 * computes lrp_weight with the explain entry points above, then:
 *   lrp_train_step : training-mode decoder forward on the cached features, loss 0.5 CE(y, logits[:, :-1]) +
 *                    0.5 CE(y, (logits * lrp_weight)[:, :-1]) (M:95-103, :1370-1373), backward through the decoder and
 *                    the encoder (all layers trainable, M:1332-1333) -> grads_dev, losses_dev (5 floats) = what train_on_batch
 *                    returns: total, loss head 1, loss head 2, accuracy head 1, accuracy head 2 (M:105-124).  A row counts
 *                    as a hit when its label's logit is >= the row maximum; tf.argmax takes the first maximal index, so the
 *                    two differ only on an exact tie at the maximum (with grid-TD's logits Dropout: a tie at 0).
 *   (the host all-reduces grads_dev across ranks)
 *   lrp_train_apply: Adam(lr, clipvalue) as keras does (clip element-wise, then the moments; epsilon 1e-7) on the fp32
 *                    master weights; the engine's operand copies are rebuilt, cached images are dropped.
 * All parameters live in one flat fp32 buffer: lrp_train_num_params / lrp_train_param_info give name, offset and size
 * of each slice ("<layer>_W" HWIO, "<layer>_b", then the decoder weights under their lrp_set_weight names);
 * grads_dev has the same layout, lrp_train_flat_size floats.  cap_in_dev (B, T) int32 embedding rows (the model's
 * `captions_input`), y_idx_dev (B, T) int32 class index of the one-hot label row or -1 for an all-zero row,
 * lrp_weight_dev (B, T, V) float32.  Dropout masks (values 0 or 1/(1-p)) or NULL: image_features (B, L, H),
 * global (B, E), output (B, T, H); LSTM-cell dropout (keras `dropout` / `recurrent_dropout`, one mask per gate i f c o
 * and per step because the wrapper calls the cell inside the K.rnn loop, M:582): lstm_in (T, 4, B, 2E),
 * lstm_rec (T, 4, B, H) (for grid-TD the language LSTM: lstm_in (T, 4, B, 2H)); logits (B, T, V): the grid-TD model's
 * Dropout on the logits (M:1303-1304), NULL for the adaptive model. */
int lrp_train_begin(lrp_handle* h, float lr, float clipvalue, float beta1, float beta2, float eps);
/* ABI v3.  Arithmetic of the step's convolution gradients (BASELINE config 5 names bf16; models/model.py:1340-1374 is
 * float32 in the reference).  Master weights, Adam and every accumulation are fp32 in both modes.
 *   LRP_TRAIN_FP32 (default)  weight gradients on the fp32 MFMA; backward-data convs split-bf16 (three bf16 MFMAs per
 *                             product, fp32-grade) — exact fp32 when the handle is in LRP_PREC_FP32.
 *   LRP_TRAIN_BF16            the encoder's weight gradients with bf16 operands (activations and dZ rounded to bf16,
 *                             v_mfma_f32_32x32x16_bf16, fp32 accumulate): conv weight gradients within ~1e-2 relative L1
 *                             of the fp32 ones (tests/test_gpu_train.py), 5-10x less matrix time. */
enum { LRP_TRAIN_FP32 = 0, LRP_TRAIN_BF16 = 1 };
int lrp_train_set_precision(lrp_handle* h, int32_t mode);
int64_t lrp_train_flat_size(const lrp_handle* h);
int32_t lrp_train_num_params(const lrp_handle* h);
int lrp_train_param_info(const lrp_handle* h, int32_t i, const char** name, int64_t* offset, int64_t* size);
int lrp_train_step(lrp_handle* h, int32_t B, int32_t T, const int32_t* cap_in_dev, const int32_t* y_idx_dev,
                   const float* lrp_weight_dev, const float* mask_image_features_dev, const float* mask_global_dev,
                   const float* mask_output_dev, const float* mask_lstm_in_dev, const float* mask_lstm_rec_dev,
                   const float* mask_logits_dev, float* grads_dev, float* losses_dev, void* stream);
/* Optional: the training-mode decoder forward of lrp_train_step ahead of time (it needs neither lrp_weight nor the labels),
 * e.g. on a second stream under the explanation that produces lrp_weight.  A following lrp_train_step with the same B, T
 * waits for it and starts at the loss.  Contract: the kernels read cap_in and the masks straight from the caller's device
 * buffers (nothing is staged), in the forward AND in the backward scan of lrp_train_step — so that step must be handed the
 * SAME cap_in / mask pointers (they must stay alive and unchanged until the step's work has completed); other pointers are
 * refused with LRP_ERR_INVALID rather than back-propagated through masks the forward did not use, and the refusal drops
 * the pending forward (a retry runs its own, so recycled addresses cannot pass for the old buffers).  lrp_encode_images,
 * lrp_set_features, lrp_set_weight[_dev] and lrp_set_precision drop a pending early forward. */
int lrp_train_forward(lrp_handle* h, int32_t B, int32_t T, const int32_t* cap_in_dev, const float* mask_image_features_dev,
                      const float* mask_global_dev, const float* mask_output_dev, const float* mask_lstm_in_dev,
                      const float* mask_lstm_rec_dev, void* stream);
/* ABI v6.  Forget a pending lrp_train_forward (train.py:571-577 has no counterpart: the reference runs the forward inside
 * train_on_batch).  For a caller that abandons the step it issued the early forward for — e.g. an error between the two
 * calls — and is about to release cap_in / the masks: `stream` (or, NULL, the host) first waits for the early forward, which
 * may still be reading them; the next lrp_train_step then runs its own forward.  lrp_train_step does the same by itself when
 * it refuses mismatching pointers.  No-op without a pending forward. */
int lrp_train_drop_forward(lrp_handle* h, void* stream);
int lrp_train_apply(lrp_handle* h, const float* grads_dev, void* stream);
int lrp_train_get_master(lrp_handle* h, float* flat_dev, void* stream);

/* ABI v4.  Kernel launches issued by this library since it was loaded (all handles, this process; copies and memsets not
 * counted): bench.py brackets one single-image explanation with it (`latency.launches`). */
int64_t lrp_launch_count(void);

/* ABI v6.  The library's A/B switches (LRP_CONV_HALO, LRP_UP2_PW, LRP_IMG_FOLD, ... — measurement knobs and
 * tested fall-backs, every one exercised by tests/test_gpu_switches.py) are read from the environment once per process, not on
 * the launch path; this re-reads them.  For tests and measurement scripts: call it between launches, never while another
 * thread is inside the library.  A switch that changes how lrp_encode_images lays out its caches takes effect at the next
 * lrp_encode_images.  The reference has no counterpart. */
int lrp_reload_switches(void);

/* ABI v8.  Which form of the implicit-GEMM convolution kernel a launch would take (csrc/conv_plan.h conv_plan: the one
 * function the launcher executes and every caller inside the library asks) — pure host arithmetic on the current switches:
 * it touches no device, so the tile rules can be tested on a machine without a GPU (tests/test_conv_plan.py).
 *   epi    LRP_EPI_*: the epilogue;  prec  LRP_OPND_*: the operand format;  terms  7, or 5 / 23 (two-MFMA forms of LRP_OPND_F16X2)
 *   NB, H, W   the image stack (a 1-tap GEMM: NB rows, H = W = 1);  N output columns from Cin channels;  taps 9 or 1
 *   split  LRP_EPI_FWD_DUAL: the columns of the first half
 *   flags  LRP_PLAN_FRAG ... GMASK: facts about the operands;  LRP_PLAN_UP2_SRC / IMG_PART / POOL_GC: what the caller wants the
 *          launch to carry (compact pool interface, folded image layer, pool fused into the dual forward) — only some forms can
 *   out11  ok, form (LRP_FORM_*), BM, BN, threads, tw, th, hrows, tpt, m_tiles, n_tiles;  ok = 0: the launch would be refused
 * A request is carried by a resident-image form or refused, never dropped: IMG_PART with fp32 operands is refused (no kernel
 * of that format reads it), and under LRP_CONV_HALO=2 a launch with a request is still decided at the default fill of 0.9.
 * LRP_FORM_BREG4 / LRP_FORM_BREG4_POOL: the 128 x 128 tile and geometry of LRP_FORM_HALO / LRP_FORM_POOL on the loop that takes its
 * weights from registers (one workgroup barrier per channel chunk) — with LRP_PLAN_FRAG and N % 128 == 0, for the dense split-bf16
 * LRP_EPI_MUL launch (no JOIN, no request) and the interleaved fp16-pair LRP_EPI_FWD_DUAL (terms 7 | 23; POOL_GC gives the _POOL
 * form).  LRP_CONV_BREG4=0 gives the pipelined forms back.
 * LRP_FORM_BREG (N <= 64, 128 x 64 tile, weights in registers) names two loops of one kernel family; which one a launch runs on is the
 * launcher's choice and no part of this answer: the chunk loop of LRP_FORM_BREG8 / BREG4 for the dense split-bf16 LRP_EPI_MUL
 * launch, the tile's first loop for everything else and under LRP_CONV_BREG2=0.  Every field here is the same under both settings.
 * LRP_PLAN_DUAL_MUL (added later in ABI v10): the dual-gate epilogue of the alpha-beta walk (two gates on one accumulator, two outputs; Cin counts both
 * chains).  LRP_EPI_MUL / LRP_EPI_MUL_UP2 with LRP_OPND_FP32 or LRP_OPND_BF16X3 on LRP_FORM_PLAIN, LRP_FORM_SMALL and the 128 x 128
 * LRP_FORM_HALO; never the 8-wave tile or a weights-in-registers form; refused with FRAG, JOIN, GMASK, any request, LRP_OPND_F16X2,
 * or chains that are not whole 16 B (fp32) / 32 B (split) groups.
 * The reference has no counterpart. */
enum { LRP_EPI_BIAS_RELU = 0, LRP_EPI_BIAS = 1, LRP_EPI_MUL = 2, LRP_EPI_MUL_UP2 = 3, LRP_EPI_FWD_DUAL = 4, LRP_EPI_STORE = 5,
       LRP_EPI_IMG_STENCIL = 6 };
enum { LRP_OPND_FP32 = 0, LRP_OPND_BF16X3 = 1, LRP_OPND_F16X2 = 2 };
enum { LRP_FORM_PLAIN = 0, LRP_FORM_SMALL = 1, LRP_FORM_HALO = 2, LRP_FORM_BREG = 3, LRP_FORM_POOL = 4, LRP_FORM_IMG = 5, LRP_FORM_BREG8 = 6,
       LRP_FORM_BREG4 = 7, LRP_FORM_BREG4_POOL = 8 };
enum { LRP_PLAN_FRAG = 1, LRP_PLAN_JOIN = 2, LRP_PLAN_DUAL_IL = 4, LRP_PLAN_GMASK = 8,
       LRP_PLAN_UP2_SRC = 16, LRP_PLAN_IMG_PART = 32, LRP_PLAN_POOL_GC = 64, LRP_PLAN_DUAL_MUL = 128 };
int lrp_conv_plan(int32_t epi, int32_t prec, int32_t terms, int32_t NB, int32_t H, int32_t W, int32_t N, int32_t Cin, int32_t taps,
                  int32_t split, uint32_t flags, int32_t* out11);

const char* lrp_last_error(void);
int lrp_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_H */
