// conv_args.h — what a launch of conv_igemm_kernel (conv_igemm.h) is told: the operand formats and epilogues, the kernel's
// argument block and the constants the kernel, its launch plan (conv_plan.h) and the passes around it (cnn_kernels.h) share.
#pragma once

// ---- plain C++: conv_plan.h includes this file and compiles without HIP ----
namespace lrp {

// PREC_FP32 : operands fp32, v_mfma_f32_32x32x2_f32 (exact fp32 fma chain).  The walk and the forward of LRP_PREC_FP32; the image
//   layer's forward GEMM and the decoder's products in every mode.
// PREC_BF16X3: operands stored as "split8" — per 8 consecutive channels 32 B = [8 x bf16 hi | 8 x bf16 lo] with
//   x ~= hi + lo (16 mantissa bits), same bytes as fp32.  Each product is hi*hi' + hi*lo' + lo*hi' on
//   v_mfma_f32_32x32x16_bf16 with fp32 accumulation: 3 MFMAs of 32 cycles per 16 k instead of 8 of 64
//   (5.3x fewer matrix-pipe cycles).  The per-token reverse walk of the DEFAULT mode (lrp_create: LRP_PREC_BF16X3): worst case
//   2^-16 per product whatever the weights [MI355X: 2-3.5e-6 relative L1 vs the float64 graph on He-normal kernels,
//   6e-6 ... 1.6e-5 on trained-like ones, DESIGN 4.2].
// PREC_F16X2 : both operands as fp16 pairs hi + lo (22 mantissa bits) in the same split8 layout, carried scaled by powers
//   of two taken from MEASURED maxima (fp16 has 5 exponent bits): per token for the relevance S of the reverse walk
//   (ConvArgs::tok_*; Encoder::explain), per image for the forward's activations, per matrix for the weights.
//   TERMS 7: hi*hi' + hi*lo' + lo*hi', three v_mfma_f32_32x32x16_f16 per 16 k — fp32-grade.  This is the encoder FORWARD of every
//   mode but LRP_PREC_FP32 (the interleaved dual conv a_l | Z+_l, blocked accumulation: features 7e-7 from float64) and the top
//   block of the opt-in fast walk.
//   TERMS 5: the weights' lo half is not read: lo*w + hi*w, TWO MFMAs — the layers of the OPT-IN fast walk (LRP_PREC_F16X2) that
//   lrp_set_fast_layers / calibration.py selected; TERMS bit 4 computes the matching two-term denominators Z+ in the forward.
//   One fp16 per weight is 2^-12 per product: fine on dense Gaussian kernels (the rounding averages out), above the 1e-4 bar on
//   sparse heavy-tailed ones — which is why this is not the default (tests/test_gpu_stress_parity.py).
enum ConvPrec { PREC_FP32 = 0, PREC_BF16X3 = 1, PREC_F16X2 = 2 };

enum ConvEpi {
  EPI_BIAS_RELU = 0,  // out = relu(acc + bias)
  EPI_BIAS = 1,       // out = acc + bias
  EPI_MUL = 2,        // out = acc * aux[img(row)]               (conv-LRP, no pool)
  EPI_MUL_UP2 = 3,    // out(2x res) = acc * aux[img(row)](2x)   (conv-LRP through a 2x2 max-pool)
  EPI_FWD_DUAL = 4,   // cols [0,split): out = relu(acc+bias); cols [split,2split): out2 = acc+bias  (a_l and Z+_l)
  EPI_STORE = 5,      // out = acc (row stride = N)   (image layer: tap-expanded channel reduction, see img_stencil_kernel)
  // Image layer in ONE launch: the rows of a tile are a 16 x 16 pixel PATCH (14 x 14 output pixels + 1 halo), the
  // tile computes T = S_1 . W (54 tap-expanded columns, see cnn_kernels.h) for the patch, keeps it in LDS and applies
  // the 9-tap shift-and-add for its 14 x 14 interior: S_1 is read once (x 1.31 halo) and only R_img is written,
  // instead of writing and re-reading the 3.5 GB T tensor.  BM = 256, BN = 64, 1 tap.
  EPI_IMG_STENCIL = 6
};
constexpr int IMG_PATCH = 16, IMG_TILE = 14;
constexpr int ACT_MAX_SLOTS = 64;

constexpr int LDS_STRIDE = 32;   // floats per staged row (128 B, no padding; swizzled chunks)

// HALO (3x3 only): instead of re-staging the A tile for each of the 9 taps (9 x BM rows per 32-channel
// chunk, 8 of them L2 hits but still L2->LDS traffic, the limiter of the bf16x3 mode), the tile's pixels
// PLUS their one-pixel halo are staged once per channel chunk and the taps read shifted rows of that
// resident image.  A traffic per chunk: 9 x 256 rows -> 352 rows.
// The resident image is a window of the EXTENDED stack: every image contributes its H rows plus one all-zero
// separator row (extended row E = n*(H+1) + h, h == H is the separator), and columns x0-1 .. x0+tw with zeros
// outside [0, W).  A pixel's 3x3 neighbourhood is then always at fixed offsets (dy*HALO_PITCH + dx) from it,
// borders included: no per-lane tap masks in the main loop.  See DESIGN.md 4.1.
constexpr int HALO_PITCH = 16, HALO_PL = 4;
constexpr int conv_halo_rows(int BM) { return BM == 256 ? 352 : 192; }   // x 128 B; 22 / 12 image rows

}  // namespace lrp

#if defined(__HIPCC__)   // ---- the device-side types: HIP translation units only ----
#include <hip/hip_runtime.h>
#include <vector>

namespace lrp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split8h_store(const float* r, float* dst) {  // 8 fp32 -> 32 B [fp16 hi8 | fp16 lo8]
  f16x8 hi, lo;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    hi[q] = (_Float16)r[q];
    lo[q] = (_Float16)(r[q] - (float)hi[q]);
  }
  u32x4* d = reinterpret_cast<u32x4*>(dst);
  d[0] = __builtin_bit_cast(u32x4, hi);
  d[1] = __builtin_bit_cast(u32x4, lo);
}
__device__ __forceinline__ void split8_store(const float* r, float* dst) {   // 8 fp32 -> 32 B [hi8 | lo8]
  bf16x8 hi, lo;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    hi[q] = (__bf16)r[q];
    lo[q] = (__bf16)(r[q] - (float)hi[q]);
  }
  u32x4* d = reinterpret_cast<u32x4*>(dst);
  d[0] = __builtin_bit_cast(u32x4, hi);
  d[1] = __builtin_bit_cast(u32x4, lo);
}
// exact small-integer division (operands < 2^22): float estimate + one fix-up step
__device__ __forceinline__ void conv_divmod(int x, int d, float inv, int& q, int& r) {
  q = (int)(((float)x + 0.5f) * inv);
  r = x - q * d;
  if (r < 0) { --q; r += d; } else if (r >= d) { ++q; r -= d; }
}

// Halo-resident launches walk the image STACK (all tokens on top of each other) tile row by tile row.  The gate a tile is
// multiplied with belongs to the token's IMAGE, and with several tokens per image (10 words per caption) the same gate rows
// were fetched once per token — the stack order puts 25 tile rows of other traffic between two uses, far more than an
// XCD's 4 MB of L2 [MI355X, block1_conv2: FETCH_SIZE 8.2 GB = S_in 4.1 + 10 x 0.41 of gates].  TileOrder is a per-layer
// host cache of a permutation of the tiles — ordered by (image, column strip, row band, token) — so that the tiles of an
// image's tokens at the same place run back to back on one XCD (they share the gate rows in its L2) and a strip's next
// row band follows within a few dozen tiles (the vertical halo rows of S are still there); built from the call's
// token -> image map, rebuilt only when that map changes.  Tiles are independent, so the order changes no result bit.
struct TileOrder {
  std::vector<int> sig;                                 // token -> image map the table was built for
  int H = 0, th = 0, nyh = 0, cols_t = 0, tpt = 0;
  bool identity = true;
  int* dev = nullptr;
  int* pinned = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;                              // the last upload
  TileOrder() = default;
  TileOrder(const TileOrder&) = delete;
  TileOrder& operator=(const TileOrder&) = delete;
  ~TileOrder() {
    if (dev) (void)hipFree(dev);
    if (pinned) (void)hipHostFree(pinned);
    if (ev) (void)hipEventDestroy(ev);
  }
};

struct ConvArgs {
  const float* in;     // [NB][H][W][Cin] fp32
  const float* wpk;    // [n_tiles*BN][K] fp32, K = taps*CinP, CinP = roundup(Cin,32), zero padded
  const float* wpk_frag;  // BREG: the same weights fragment-major, [kc][step][hi|lo][lane half][all N columns] x 16 B (N = 64, or N % 128 == 0)
  int NB, H, W, Cin, CinP;
  int N;               // valid output columns
  int taps;            // 9 (3x3 same) or 1
  int M;               // NB*H*W
  int m_tiles, n_tiles;
  const float* bias;
  float* out;
  float* out2;
  const float* aux;
  const int* row2img;  // per input image-slot n -> cache slot (nullptr = identity)
  int split;
  int out_plain;       // bf16x3 MUL epilogues: 1 = write fp32 instead of re-splitting (last GEMM of a chain)
  // EPI_IMG_STENCIL: tiles per image row / column, ximg = the images (x of the image layer), mode 0 LRP | 1 sum | 2 x*sum |
  // 3 bounded: (x - img_lo) * sum+ + (x - img_hi) * sum-  (the two bounds are the struct's last members)
  int tiles_x, tiles_y, img_mode;
  const float* ximg;
  const float* addend; // BIAS / BIAS_RELU epilogues: out = [relu](acc + bias + addend)  (bias may be null)
  // EPI_BIAS only: out = gate_src / SafeDivide-denominator(acc + bias) — the relevance gate G_l = a_l / safe(Z+_l)
  // (IL:456-458) straight from the denominator conv, Z+_l itself never goes to memory.  gate_src may alias out (the
  // overlapped encode parks a_l in the gate's storage): an element is read and written by the same thread.
  const float* gate_src;
  // EPI_MUL only — tail of a residual block in one epilogue (ResNet walk):
  //   r    = acc * aux[img] + join[row] * join_gate[img]     (the shortcut's share joins the main branch, KG:799-803)
  //   out  = r                                               (fp32 / split8 as usual)
  //   out2 = r * gate2[img]                                  (head of the NEXT block's conv chain; split8 in bf16x3 mode)
  const float* join;
  const float* join_gate;
  const float* gate2;
  float* out2s;
  // gradient baselines on the MUL epilogues: the cached LRP gate is used as a MASK (gate != 0 <=> the unit's ReLU was
  // active and it won its pool window), and guided backprop also clamps the propagated value at 0
  int gate_binary, relu_out;
  int dual_norelu;     // EPI_FWD_DUAL: first half without the relu (a conv + BatchNorm unit: c and Z+ in one pass)
  // EPI_FWD_DUAL, interleaved weights (dual_il): the stacked matrix has its rows in blocks of 32 — [w of channels 32g..32g+31 |
  // w+ of the SAME channels] — so a tile holds c and Z+ of a channel side by side and the epilogue can finish the pair:
  // dual_gate = 1: out = a_l = relu(c), out2 = the relevance gate G_l = a_l / safe(Z+_l) (IL:456-458); Z+_l never goes to
  // memory and no gate pass follows.  dual_gate = 0: out2 = Z+_l as in the stacked form.  Needs split % 32 == 0.
  int dual_il, dual_gate;
  // dual_gate = 2 (a conv + BatchNorm unit of the ResNet encoder, RA:197-257 folded with alpha1beta0; resnet_kernels.h
  // rn_bn_unit_kernel is the unfused form): with c = conv + b, Z = the alpha1beta0 denominator,
  //   y = gamma (c - mean) / sqrt(var + eps) + beta,  Q = c (y - beta) / stab((c - mean) y) / safe(Z)
  //   bn_relu: out = relu(y), out2 = relu(y) Q      else: out = y, out2 = Q
  const float* bn_gamma; const float* bn_beta; const float* bn_mean; const float* bn_var;
  float bn_eps; int bn_relu;
  // halo-resident 3x3 variant (template HALO): a tile is th rows x tw (<= 14) columns of the image stack
  // (all NB images on top of each other: Y = n*H + h), cols_t tiles per image row; hrows = rows of the
  // resident image (th + 2 + separator rows), each HALO_PITCH pixels wide
  int tw, th, hrows, cols_t, nyh;
  const int* tile_map;        // device: launch position -> tile of the stack (nullptr = stack order); filled by the launcher from:
  TileOrder* order;           // host: the layer's cache (nullptr = never reorder)
  const int* row2img_host;    // host copy of row2img for this call (nullptr = identity: one token per image)
  // PREC_F16X2: per-token power-of-two scaling of the fp16 relevance tensors (indexed by the token slot n of a row).
  //   stored input = true * 2^e_in[n], |stored input| <= max_in[n] (measured by the producer).  tok_scale_kernel
  //   (cnn_kernels.h) picks k[n] = floor(log2(30000 / (max_in[n] * wnorm))) — wnorm = max row sum of |w| of the layer's
  //   backward matrix, the gate is <= 1, so |acc * gate| * 2^k stays below fp16's 65504 — and hands this launch
  //   tok_fac[n] = 2^k[n]; the epilogue stores acc * gate * tok_fac[n] and raises tok_max_out[n] (float bits) to the
  //   largest |stored output|.  EPI_IMG_STENCIL ends the chain: tok_fac[n] = 2^-e_in[n].
  const float* tok_fac;
  unsigned* tok_max_out;
  // PREC_F16X2 forward (EPI_BIAS / EPI_BIAS_RELU, TERMS 7 = fp16 pairs on BOTH operands, 22 mantissa bits: an fp32-grade
  // product in three MFMAs): the input tensor is stored scaled by a power of two; *in_unscale (device scalar) = its
  // inverse, applied to the accumulator in front of the bias.  act_max_out: ACT_MAX_SLOTS float-bit slots raised to the
  // largest |out| (slot = block id mod slots: spreads the atomics; the consumer takes the maximum over the slots).
  const float* in_unscale;
  unsigned* act_max_out;
  // EPI_FWD_DUAL, interleaved rows, PREC_F16X2: the epilogue also writes a_l as the NEXT conv's operand — fp16 pairs
  // [hi8 | lo8] of a_l * *pairs_scale (a power of two chosen BEFORE the launch from a bound on |a_l|: the measured maximum
  // of this conv's input x its weights' largest absolute row sum + max|b|; cnn_kernels.h fwd_scale_kernel) — so no split
  // pass runs between two convs.  skip_out: a_l itself (fp32) is not written (nobody else reads it).
  float* pairs_out;
  const float* pairs_scale;
  int skip_out;
  // scale_per_img (interleaved dual forward): in_unscale, pairs_scale and act_max_out are arrays indexed by the IMAGE of a row
  // (row / img_rows; act_max_out[image][ACT_MAX_SLOTS]) instead of one record for the call — an image's rows only ever gather
  // from that image, so a scale per image is as legal as one per call, and the result for an image no longer depends on
  // which other images share its batch.
  int scale_per_img, img_rows, n_imgs;
  // Compact pool interface (PREC_BF16X3, EPI_MUL / EPI_MUL_UP2 on the halo kernels: the folded weights-in-registers launch and
  // the pipelined 128 x 128 / 256 x 256 tiles): the relevance entering this layer came through a 2x2 max-pool, i.e.
  // S_in[n][y][x][c] = S_c[n][y/2][x/2][c] at the window's arg-max position and 0 at the three others.  Instead of reading that
  // 4x-expanded, 75 %-zero tensor (which its producer would have had to write), the producer runs EPI_MUL with this layer's
  // COMPACT pool gate and writes S_c = acc x gate at pooled resolution as bf16 pairs, and the tile builds its resident image
  // from S_c and the position bytes (2 dy + dx per window and channel, per image: shared by an image's tokens in L2): the
  // value where the position matches, zeros elsewhere.  `in` is then unused.
  const float* up2_src;        // S_c [NB][H/2][W/2][Cin] split8 bf16 pairs
  int gate_none;               // EPI_MUL: out = acc, no gate (ResNet gradient walk: a unit without a ReLU mask in front)
  const unsigned char* up2_gpos;   // [images][H/2][W/2][Cin] bytes
  int up2_pairs;               // must be 1 with up2_src: pairs are the only form the loaders read (conv_launch_epi refuses others)
  // Image layer folded into the epilogue of the layer above it (weights-in-registers kernel, PREC_BF16X3, N = 64, EPI_MUL):
  // S_1 = acc x gate never goes to memory.  The tile turns it into bf16 pairs in LDS, multiplies it with the tap-expanded
  // 64 -> 54 matrix `img_w` (the image layer's T = S_1 . W, cnn_kernels.h) and applies the 9-tap shift-and-add for the
  // SOURCE pixels it owns: per tile (th + 2) x (tw + 2) output positions (its pixels and the one-pixel ring around them)
  // x 6 partial sums go to img_part[tile of the stack][position][6]; img_partial_sum_kernel adds the up to four tiles'
  // partials of a pixel in a fixed order and applies x+ / x-.  Tiles are laid out per token (tpt below: none straddles two
  // tokens, so the grouping of a pixel's nine taps into partials is the same for every token and every batch: results stay
  // batch-invariant bit for bit).
  const float* img_w;          // [64][64] split8 bf16 pairs (layer 0's backward matrix)
  float* img_part;
  // tpt > 0 (folded launch): tiles are laid out PER TOKEN — tpt tile rows of th stack rows per token, the last one possibly
  // short — instead of over the whole stack, so that no tile straddles two tokens and the tile boundaries fall at the same
  // image rows for every token.  Tile row R of the launch covers token R / tpt, image rows (R % tpt) * th ...
  int tpt;
  int epi_generic;             // MUL / MUL_UP2 epilogues: 1 = always the general pass loop (A/B switch LRP_EPI_FAST=0; filled by the launcher)
  // 2x2 max-pool fused into the interleaved dual forward's epilogue (PREC_F16X2, 128 x 128 resident-image tile: the whole C
  // tile is in LDS; tiles of an EVEN number of rows and columns starting at even positions, so a window never straddles two
  // tiles): per window and channel the epilogue takes the first maximum in scan order, and writes — instead of a_l and Z+_l
  // at full resolution, which a streaming pass then read back (cnn_kernels.h pool_gate_split_kernel: the same arithmetic) —
  //   pool_gc   [images][H/2][W/2][C]   the gate a_l / safe(Z+_l) at the winning position (IL:456-458 through the pool)
  //   pool_pos  same shape, bytes        that position, 2 dy + dx
  //   pairs_out [images][H/2][W/2][C]   the pooled activation as the next conv's fp16 pairs (x pairs_scale[image])
  //   pool_x    (optional) the pooled activation in fp32
  // and raises act_max_out from the pooled values.  The full-resolution gate is rebuilt from (pool_gc, pool_pos) on demand.
  float* pool_gc;
  unsigned char* pool_pos;
  float* pool_x;
  // Dual-gate MUL epilogues (template DG; alpha-beta LRP with beta > 0, Encoder::explain_table): the two relevance chains
  // S+ = R / safe(Z_act) and S- = R / safe(Z_inh) travel as ONE tensor, channels [S+ (C) | S- (C)] per pixel, so that the
  // launch against the concatenated matrix [alpha w+ ; -beta w-] (K = taps x 2C) is the ordinary implicit GEMM with
  // Cin = 2C and its accumulator c = convT(S+, alpha w+) + convT(S-, -beta w-) is shared by both chains:
  //   out = c x aux[img],  out_b = c x aux_b[img]      (aux = G+ = a / safe(Z_act), aux_b = G- = a / safe(Z_inh): N wide each)
  // out / out_b have ostride floats per pixel (2N with out_b = out + N: the next launch's input; N for two plain tensors).
  const float* aux_b;
  float* out_b;
  int ostride;
  float img_lo, img_hi;        // EPI_IMG_STENCIL, img_mode 3 (BoundedRule at the image layer): the bounds (low, high)
};

}  // namespace lrp
#endif
