// conv_plan.h — the launch plan of conv_igemm_kernel (conv_igemm.h): which instantiations of the kernel exist, which of them a
// convolution runs on, and which layers need a fragment-major weight copy for it.  Host code in plain C++ (no HIP): the kernel's
// static_assert, the launchers (conv_launch.h), the encoders and lrp_conv_plan (include/lrp_hip.h) all read the answers here.
#pragma once
#include "conv_args.h"
#include "switches.h"

namespace lrp {

// tile configurations: (WM,WN,TM,TN) -> BM x BN
//   big   : 2,2,2,2 -> 128 x 128   (N >= 128)                 64 KB LDS, 2 blocks/CU   [fp32]
//   n64   : 2,2,2,1 -> 128 x  64   (N == 64 layers)           48 KB LDS, 3 blocks/CU
//   n32   : 4,1,1,1 -> 128 x  32   (N <= 32: tiny test nets)  40 KB LDS
//   big, BREG (FORM_BREG4): weights in registers, 64 KB LDS, 2 blocks/CU   [dense bf16x3 walk, interleaved f16x2 dual forward; N % 128 == 0]
//   w256  : 2,4,4,2 -> 256 x 256   8 waves, 128 KB LDS, 1 block/CU   [bf16x3, N % 256 == 0; BREG: the dense walk launches, FORM_BREG8]
// bf16x3 spends 5.3x fewer matrix cycles per byte staged, so its limiter is the L2 -> LDS path
// (~43 GB/s per CU at 128 x 128): the 8-wave tile stages 50 % fewer bytes per FLOP.
struct ConvTile { int BM, BN; };
inline ConvTile conv_pick_tile(int N) {
  if (N > 64) return {128, 128};
  if (N > 32) return {128, 64};
  return {128, 32};
}
inline int conv_npad(int N) { ConvTile t = conv_pick_tile(N); return (N + t.BN - 1) / t.BN * t.BN; }
inline int conv_cinp(int Cin) { return (Cin + 31) / 32 * 32; }

// ---- the launch plan: ONE host function decides which form of conv_igemm_kernel a convolution runs on ----
// conv_launch_epi executes the plan; a caller that has to know what a launch will do BEFORE it launches (Encoder::explain:
// may the producer write the compact pool interface, may the image layer ride on this launch; Encoder::encode: may the pool be
// fused) asks conv_plan about that launch with its request set and reads `ok`.  lrp_conv_plan (include/lrp_hip.h) exposes it.
enum ConvForm {
  FORM_PLAIN = 0,   // A and B staged per k-step, 128 x 128 / 128 x 64 / 128 x 32 / 8-wave 256 x 256
  FORM_SMALL = 1,   // small grids: 64 x 64 tiles, CONV_SMALL_NS-stage k pipeline
  FORM_HALO = 2,    // resident image (3x3, split operands), 128 x 128 / 128 x 64 / 8-wave 256 x 256
  FORM_BREG = 3,    // resident image + weights in registers (N <= 64), 128 x 64; two loops: the launcher's choice (LRP_CONV_BREG2, conv_launch.h)
  FORM_POOL = 4,    // FORM_HALO 128 x 128 with tiles of even height and width: the 2x2 max-pool in the dual forward's epilogue
  FORM_IMG = 5,     // EPI_IMG_STENCIL: 16 x 16 pixel patches
  FORM_BREG8 = 6,   // FORM_HALO's 8-wave 256 x 256 tile with the weights in registers (dense split-bf16 EPI_MUL, N % 256 == 0)
  FORM_BREG4 = 7,   // FORM_HALO's 128 x 128 tile with the weights in registers (N % 128 == 0: dense split-bf16 EPI_MUL, interleaved fp16-pair dual forward)
  FORM_BREG4_POOL = 8   // FORM_POOL's even tiles on the FORM_BREG4 loop
};
// one launch, as far as the decision depends on it.  The three requests are what the caller wants this launch to CARRY
// (ConvArgs::up2_src, img_part, pool_gc): only some forms can, and a request never changes the tile — it is refused instead.
struct ConvAsk {
  int epi = EPI_MUL, prec = PREC_FP32, terms = 7;
  bool gmask = false;
  int NB = 0, H = 0, W = 0, N = 0, Cin = 0, taps = 9;
  bool frag = false;         // a fragment-major copy of the weights exists (ConvArgs::wpk_frag)
  bool join = false;         // ConvArgs::join
  bool dual_il = false;
  int split = 0;
  bool up2_src = false, img_part = false, pool_gc = false;
  bool dual_mul = false;     // the dual-gate MUL epilogue (ConvArgs::aux_b; Cin = both chains)
};
struct ConvPlan {
  bool ok;                   // false: conv_launch refuses this launch (hipErrorInvalidValue)
  int form, BM, BN, threads;
  bool pw;                   // FORM_BREG4 reading the compact pool interface: the kernel's PW axis
  int M, m_tiles, n_tiles, tw, th, hrows, cols_t, nyh, tpt, epi_generic;   // what the launcher writes into ConvArgs
};

constexpr int CONV_SMALL_NS = 4;                       // LDS stages of the 64 x 64 tile's k pipeline (4 x 16 KB: two workgroups per CU... see NS)
// Small grids take 64 x 64 tiles up to a 128-row grid of 128 tiles (4x as many 64 x 64 workgroups = the 512 that are resident
// at once; beyond that a second round of small tiles costs more than the large tiles' idle CUs [MI355X, one image, 252 large
// tiles: 115 -> 145 us]); up to twice that, 128 x 64 tiles.
constexpr long CONV_SMALL_BLOCKS = 128;

// ---- which instantiations of conv_igemm_kernel exist: the ONE statement ----
// conv_plan refuses what has no kernel through these functions, conv_launch / conv_launch_epi (conv_launch.h) instantiate exactly
// what they accept, and the kernel's static_assert refuses every other combination of template arguments.  A new kernel form, or
// an epilogue on a form that lacks it, is stated here and nowhere else.
//
// 1. The (epilogue, operand format, terms) that exist, whatever the form.  Exact fp32: every epilogue (TERMS is not read: 7).
// PREC_BF16X3: the reverse-walk epilogues (MUL, MUL_UP2, STORE, the image stencil) and the forward Z+ / late activation convs
// (BIAS, BIAS_RELU), always three-term.  PREC_F16X2: see TERMS (conv_igemm.h) — 7 everything but STORE, 5 the MUL epilogues, 23
// the dual forward.  gmask (byte-mask gates): exact fp32 EPI_MUL only.  dual (the dual-gate epilogue, alpha-beta LRP with
// beta > 0): the MUL epilogues in exact fp32 and split-bf16; no fp16 pairs, no byte masks.
constexpr int CONV_TERMS[] = {7, 5, 23};               // every value of the TERMS axis
constexpr bool conv_epi_exists(int epi, int prec, int terms, bool gmask, bool dual) {
  const bool mul = epi == EPI_MUL || epi == EPI_MUL_UP2;
  if (epi < EPI_BIAS_RELU || epi > EPI_IMG_STENCIL) return false;
  if (gmask && !(epi == EPI_MUL && prec == PREC_FP32 && !dual)) return false;
  if (dual && !(mul && prec != PREC_F16X2)) return false;
  switch (prec) {
    case PREC_FP32: return terms == 7;
    case PREC_BF16X3: return terms == 7 && epi != EPI_FWD_DUAL;
    case PREC_F16X2: return terms == 7 ? epi != EPI_STORE : terms == 5 ? mul : terms == 23 && epi == EPI_FWD_DUAL;
  }
  return false;
}
// the TERMS a launch is instantiated with: a single-gate exact-fp32 launch takes any request (its kernels read none)
constexpr int conv_terms(int prec, int terms, bool dual) { return prec == PREC_FP32 && !dual ? 7 : terms; }

// 2. The forms and tiles, and which of the above each has.  pw: the launch reads the compact pool interface (ConvArgs::up2_src)
// through the kernel's PW axis — FORM_BREG4 only; the pipelined tiles decide that at run time.
//   FORM_PLAIN / FORM_SMALL   everything (the 8-wave tile: split operands, one gate)
//   FORM_HALO                 split operands, the MUL and forward epilogues; dual gate: split-bf16 on the 128 x 128 tile
//   FORM_BREG                 the MUL epilogues, both split formats; the dense split-bf16 walk (EPI_MUL, PREC_BF16X3) also on the
//                             chunk loop (c2), there with the PW axis
//   FORM_BREG8                the dense split-bf16 walk: EPI_MUL, PREC_BF16X3
//   FORM_BREG4                the same, and the fp16-pair dual forward (TERMS 7 / 23)
//   FORM_POOL, FORM_BREG4_POOL   the fp16-pair dual forward (the kernels of FORM_HALO 128 x 128 / FORM_BREG4)
// Not built, and refused: a dual gate on the 8-wave tile or on a weights-in-registers form, byte masks off the staged tiles.
// (The 8-wave tiles of the fp16-pair FORWARD epilogues are instantiated although no plan answers them — conv_plan: blocked
// accumulation does not fit that tile.)
// c2: FORM_BREG's second loop (the chunk loop of FORM_BREG8 / FORM_BREG4 on the 128 x 64 tile; LRP_CONV_BREG2) — a property of the
// kernel the launcher picks, not of the plan: the dense split-bf16 walk only, with or without the PW axis.
constexpr bool conv_kernel_exists(int form, int BM, int BN, bool pw, int epi, int prec, int terms, bool gmask, bool dual, bool c2 = false) {
  if (!conv_epi_exists(epi, prec, terms, gmask, dual)) return false;
  if (c2 && !(form == FORM_BREG && epi == EPI_MUL && prec == PREC_BF16X3 && !dual && BM == 128 && BN == 64)) return false;
  if (pw && form == FORM_BREG) return c2;
  const bool mul = epi == EPI_MUL || epi == EPI_MUL_UP2, fwd = epi == EPI_BIAS || epi == EPI_BIAS_RELU || epi == EPI_FWD_DUAL;
  const bool split = prec != PREC_FP32, walk = epi == EPI_MUL && prec == PREC_BF16X3, pairs_fwd = epi == EPI_FWD_DUAL && prec == PREC_F16X2;
  const bool t128 = BM == 128 && BN == 128, t64 = BM == 128 && BN == 64, t32 = BM == 128 && BN == 32, t256 = BM == 256 && BN == 256;
  if (pw && !(form == FORM_BREG4 && walk)) return false;
  if (epi == EPI_IMG_STENCIL || form == FORM_IMG) return epi == EPI_IMG_STENCIL && form == FORM_IMG && BM == 256 && BN == 64 && !gmask && !dual;
  switch (form) {
    case FORM_PLAIN: return t128 || t64 || t32 || (t256 && split && !dual);
    case FORM_SMALL: return BM == 64 && BN == 64;
    case FORM_HALO: return split && (mul || fwd) && (dual ? t128 : t128 || t64 || t256);
    case FORM_BREG: return split && mul && !dual && t64;
    case FORM_BREG8: return walk && !dual && t256;
    case FORM_BREG4: return (walk || pairs_fwd) && !dual && t128;
    case FORM_POOL: case FORM_BREG4_POOL: return pairs_fwd && t128;
  }
  return false;
}
// every (form, tile, pw, c2) some epilogue has a kernel for: what conv_launch_epi dispatches over
struct ConvFormTile { int form, BM, BN; bool pw, c2 = false; };
constexpr ConvFormTile CONV_FORM_TILES[] = {
    {FORM_PLAIN, 128, 128, false}, {FORM_PLAIN, 128, 64, false}, {FORM_PLAIN, 128, 32, false}, {FORM_PLAIN, 256, 256, false},
    {FORM_SMALL, 64, 64, false},   {FORM_HALO, 128, 128, false}, {FORM_HALO, 128, 64, false},  {FORM_HALO, 256, 256, false},
    {FORM_BREG, 128, 64, false},   {FORM_POOL, 128, 128, false}, {FORM_IMG, 256, 64, false},   {FORM_BREG8, 256, 256, false},
    {FORM_BREG4, 128, 128, false}, {FORM_BREG4, 128, 128, true}, {FORM_BREG4_POOL, 128, 128, false},
    {FORM_BREG, 128, 64, false, true}, {FORM_BREG, 128, 64, true, true}};
constexpr int CONV_FORM_TILE_COUNT = sizeof(CONV_FORM_TILES) / sizeof(CONV_FORM_TILES[0]);

// the kernel's template arguments for a (form, tile, pw): BM = 32 WM TM, BN = 32 WN TN; see the tile configurations above
struct ConvKernelShape { int WM, WN, TM, TN; bool HALO, BREG; int NS; bool PW, C2 = false; };
constexpr ConvKernelShape conv_kernel_shape(int form, int BM, int BN, bool pw, bool c2 = false) {
  const bool breg = form == FORM_BREG || form == FORM_BREG8 || form == FORM_BREG4 || form == FORM_BREG4_POOL;
  const bool halo = breg || form == FORM_HALO || form == FORM_POOL;
  const int ns = form == FORM_SMALL ? CONV_SMALL_NS : 2;
  if (form == FORM_IMG) return {4, 1, 2, 2, false, false, 2, false};                      // 256 x 64: a 16 x 16 pixel patch
  if (BM == 256) return {2, 4, 4, 2, halo, breg, ns, pw};
  if (BM == 64) return {2, 2, 1, 1, halo, breg, ns, pw};
  if (BN == 128) return {2, 2, 2, 2, halo, breg, ns, pw};
  if (BN == 64) return {2, 2, 2, 1, halo, breg, ns, pw, c2};
  return {4, 1, 1, 1, halo, breg, ns, pw};
}
// the kernel's own question: is this set of template arguments one of the above?
constexpr bool conv_kernel_instantiated(int WM, int WN, int TM, int TN, bool HALO, bool BREG, int NS, bool PW, int epi, int prec, int terms,
                                        bool gmask, bool dual, bool C2 = false) {
  for (const ConvFormTile& f : CONV_FORM_TILES) {
    const ConvKernelShape k = conv_kernel_shape(f.form, f.BM, f.BN, f.pw, f.c2);
    if (k.WM == WM && k.WN == WN && k.TM == TM && k.TN == TN && k.HALO == HALO && k.BREG == BREG && k.NS == NS && k.PW == PW && k.C2 == C2 &&
        conv_kernel_exists(f.form, f.BM, f.BN, f.pw, epi, prec, terms, gmask, dual, f.c2))
      return true;
  }
  return false;
}

// best (tw, th, pitch) for a BM-row tile on an H x W image stack; returns the fraction of MFMA rows doing real work.
// even: an even number of rows and columns (ConvArgs::pool_gc: 2x2 windows never straddle two tiles)
inline float conv_halo_geom(int BM, int H, int W, bool even, int& tw, int& th, int& hrows) {
  const int avail = conv_halo_rows(BM) / HALO_PITCH;   // resident image rows that fit
  const int step = even ? 2 : 1;
  float best = 0.f;
  for (int c = step; c <= HALO_PITCH - 2 && c <= W; c += step) {
    // th stack rows cross at most ceil((th-1)/H) image boundaries, each costing one separator row
    int t = even ? (BM / c) & ~1 : BM / c;
    while (t > 0 && t + 2 + (t - 1 + H - 1) / H > avail) t -= step;
    if (t < step) continue;
    const int cols = (W + c - 1) / c;
    const float u = (float)(t * c) / (float)BM * (float)W / (float)(cols * c);
    if (u > best + 1e-6f) { best = u; tw = c; th = t; hrows = t + 2 + (t - 1 + H - 1) / H; }
  }
  return best;
}

// Can a reverse launch through a layer (N output columns from Cin channels at H x W) read the compact pool interface at SOME
// token count?  The part of conv_plan's answer to an up2_src request that depends on neither the grid nor a switch:
// Encoder::init sizes the compact gates by it.  (N <= 32 never reaches a kernel that reads them; those are the tiny test nets.)
inline bool conv_compact_shape(int N, int Cin, int H, int W) {
  if ((Cin & 7) || (H & 1) || (W & 1)) return false;
  return conv_pick_tile(N).BN == 128 /* pipelined halo tiles */ || (N <= 64 && conv_cinp(Cin) <= 64) /* weights in registers */;
}

// May a launch with N output columns from Cin channels take a weights-in-registers form at SOME grid — i.e. does the layer need a
// fragment-major copy of its weights (ConvArgs::wpk_frag)?  Returns the forms as bits (1 << FORM_BREG / FORM_BREG8 / FORM_BREG4;
// FORM_BREG4_POOL runs on FORM_BREG4's copy).  The part of conv_plan's weights-in-registers decisions that depends on neither
// the grid nor a request: conv_plan reads it, Encoder::alloc_conv_operands and lrp_op_conv make the copies by it.
// LRP_CONV_BREG8 / LRP_CONV_BREG4 are read here (=0: no copy is made when weights are set); LRP_CONV_BREG is a per-launch switch only.
inline unsigned conv_frag_forms(int epi, int prec, int terms, int N, int Cin, int taps, const Switches& s = sw()) {
  if (taps != 9 || N <= 0 || (Cin & 7)) return 0;        // resident-image kernels: 3x3, split operands
  auto has = [&](int form, int BM, int BN) { return conv_kernel_exists(form, BM, BN, false, epi, prec, terms, false, false); };
  unsigned forms = 0;
  if (conv_pick_tile(N).BN == 64 && has(FORM_BREG, 128, 64)) forms |= 1u << FORM_BREG;
  if (s.conv_breg8 && (N % 256) == 0 && has(FORM_BREG8, 256, 256)) forms |= 1u << FORM_BREG8;
  if (s.conv_breg4 && (N % 128) == 0 && has(FORM_BREG4, 128, 128)) forms |= 1u << FORM_BREG4;
  return forms;
}

inline ConvPlan conv_plan(const ConvAsk& q, const Switches& s = sw()) {
  const ConvPlan refused{};
  ConvPlan p{};
  const int epi = q.epi, prec = q.prec, terms = conv_terms(prec, q.terms, q.dual_mul);
  const bool mul = epi == EPI_MUL || epi == EPI_MUL_UP2, fwd = epi == EPI_BIAS || epi == EPI_BIAS_RELU || epi == EPI_FWD_DUAL;
  const bool asked = q.up2_src || q.img_part || q.pool_gc;
  // what has no kernel on any form (conv_epi_exists), and what the kernels that exist cannot be given:
  if (!conv_epi_exists(epi, prec, terms, q.gmask, q.dual_mul)) return refused;
  if (terms == 23 && !q.dual_il) return refused;                                          // two-term Z+ column blocks: interleaved rows
  if (q.gmask && asked) return refused;
  if (prec != PREC_FP32 && (q.Cin & 7)) return refused;
  // dual gate: the dense 3x3 / 1x1 launches only — no compact pool interface, no folded image layer, no residual join, and a
  // fragment-major copy of the concatenated matrix is refused, not ignored (no weights-in-registers form has the epilogue).
  // Each chain is half of Cin and must be made of whole 16 B (fp32) / 32 B (split8) groups.
  if (q.dual_mul && (asked || q.frag || q.join || (q.Cin & (prec != PREC_FP32 ? 15 : 7)))) return refused;
  const unsigned frag = q.frag ? conv_frag_forms(epi, prec, terms, q.N, q.Cin, q.taps, s) : 0;   // weights-in-registers forms this launch may take
  p.M = q.NB * q.H * q.W;
  p.epi_generic = s.epi_fast ? 0 : 1;
  ConvTile t = epi == EPI_IMG_STENCIL ? ConvTile{256, 64} : conv_pick_tile(q.N);
  // the answer: `form` on tile t — refused if this (epilogue, format, terms) has no kernel there
  auto done = [&](int form) {
    p.pw = form == FORM_BREG4 && q.up2_src;
    if (!conv_kernel_exists(form, t.BM, t.BN, p.pw, epi, prec, terms, q.gmask, q.dual_mul)) return refused;
    const ConvKernelShape k = conv_kernel_shape(form, t.BM, t.BN, p.pw);
    p.ok = true; p.form = form; p.BM = t.BM; p.BN = t.BN; p.threads = 64 * k.WM * k.WN;
    return p;
  };
  if (epi == EPI_IMG_STENCIL) {
    if (q.taps != 1 || q.N > 64 || (q.Cin & 3) || asked) return refused;
    p.n_tiles = 1;
    p.m_tiles = q.NB * ((q.W + IMG_TILE - 1) / IMG_TILE) * ((q.H + IMG_TILE - 1) / IMG_TILE);
    return done(FORM_IMG);
  }
  if (mul && (q.N & (prec != PREC_FP32 ? 7 : 3))) return refused;                         // 16 B (fp32) / 32 B (split8) epilogue
  if ((epi == EPI_BIAS || epi == EPI_BIAS_RELU) && (q.N & 3)) return refused;
  if (epi == EPI_FWD_DUAL && ((q.split & 3) || (q.dual_il && ((q.split & 31) || q.N != 2 * q.split)))) return refused;

  // ---- the tile ----
  const long rows = (long)q.NB * q.H * q.W;
  // fp32, few M rows (the per-image forward at batch 32): 128 x 128 tiles leave CUs idle; halve the tile
  // [MI355X] encode of 32 images 14.06 -> 13.54 ms with the threshold at 2200 blocks (~4 waves of 512 slots)
  if (prec == PREC_FP32 && t.BN == 128 && (q.N % 64) == 0 && ((rows + 127) / 128) * ((q.N + 127) / 128) < 2200) t = {128, 64};
  // split operands: the 8-wave 256 x 256 tile (blocked accumulation — the fp16-pair forward — does not fit it).  Measured: a
  // 256 x 128 tile loses to two 128 x 128 blocks per CU, and one 8-wave block per CU is only worth it when the grid still
  // fills the chip ~1.5 times over.  The tail of a ResNet identity block (1 tap, K = f channels, three full-width streams
  // per output element in the epilogue) is bound by those streams, not by staging: two 128 x 128 workgroups per CU overlap
  // one's epilogue with the other's K loop  [MI355X, ResNet-101 conv4_x: 354 -> 316 us per launch; config 4 -0.9 ms per walk]
  if (prec != PREC_FP32 && (q.terms == 7 || prec == PREC_F16X2) && !(prec == PREC_F16X2 && fwd) && q.N >= 256 && (q.N % 256) == 0 &&
      !(epi == EPI_MUL && q.taps == 1 && q.join) && !q.dual_mul && ((rows + 255) / 256) * (q.N / 256) >= 400)
    t = {256, 256};
  p.m_tiles = (p.M + t.BM - 1) / t.BM;
  p.n_tiles = (q.N + t.BN - 1) / t.BN;
  if (p.M <= 0 || q.N <= 0) return done(FORM_PLAIN);     // nothing to launch
  const long grid = (long)p.m_tiles * p.n_tiles;
  // the resident-image kernels exist for the split formats' 3x3 MUL and forward epilogues.  LRP_CONV_HALO=2 puts ragged tile
  // shapes on them (tests); a launch that carries a request is decided at the default fill
  const int mode = prec != PREC_FP32 && (mul || fwd) && q.taps == 9 ? s.conv_halo : 0;
  auto resident = [&](bool even, float fill) {
    int tw = 0, th = 0, hrows = 0;
    const float u = conv_halo_geom(t.BM, q.H, q.W, even, tw, th, hrows);
    if (!(u >= fill || (mode == 2 && !asked && u > 0.f))) return false;
    p.tw = tw; p.th = th; p.hrows = hrows;
    p.nyh = q.NB * q.H;
    p.cols_t = (q.W + tw - 1) / tw;
    p.m_tiles = ((p.nyh + th - 1) / th) * p.cols_t;
    return true;
  };

  if (q.pool_gc) {
    // pool fused into the dual forward's epilogue: 128 x 128 resident-image tiles of even height and width or nothing (a grid
    // small enough for the small / mid-size tiles keeps its pool pass); LRP_POOL_FUSED=0 disables
    if (epi != EPI_FWD_DUAL || prec != PREC_F16X2 || !q.dual_il || q.up2_src || q.img_part || !s.pool_fused || mode <= 0 ||
        (q.H & 1) || (q.W & 1) || t.BM != 128 || t.BN != 128 || (s.conv_small && grid <= 2 * CONV_SMALL_BLOCKS) || !resident(true, 0.8f))
      return refused;
    if (frag & (1u << FORM_BREG4)) return done(FORM_BREG4_POOL);   // (see FORM_BREG4 below)
    return done(FORM_POOL);
  }
  // N <= 64: resident image + weights in registers, no barrier per tap (LRP_CONV_BREG=0 disables).  128-row tiles, whatever
  // the grid: 256-row tiles, 8 waves, one block per CU, halve the weight traffic per pixel but lose more to the single block
  // per CU  [MI355X: block1_conv2 bwd 4.19 ms vs 3.83 ms with these 128-row tiles, 3 blocks per CU]
  if (mode > 0 && s.conv_breg && (frag & (1u << FORM_BREG)) && resident(false, 0.9f)) {
    if (q.img_part) {                                    // image layer folded in: tiles laid out per token (none straddles two tokens)
      if (prec != PREC_BF16X3 || epi != EPI_MUL || q.N != 64) return refused;
      p.tpt = (q.H + p.th - 1) / p.th;
      p.hrows = p.th + 2;                                // (no separator row inside a tile's own rows)
      p.m_tiles = q.NB * p.tpt * p.cols_t;
    }
    // (the compact pool interface needs the window loader: per-token tiles = the folded launch)
    if (q.up2_src && (!q.img_part || !conv_compact_shape(q.N, q.Cin, q.H, q.W))) return refused;
    return done(FORM_BREG);
  }
  if (q.img_part) return refused;                        // the folded image layer exists for the weights-in-registers kernel only
  // Small grids (one image, a handful of words: explain_image.py's own call): with 128-row tiles the 14 x 14 / 28 x 28
  // layers are 16-250 workgroups, each walking K = 2304-4608 alone — the launch takes as long as ONE tile's K loop
  // [MI355X, B = 1, T = 10: 115-119 us per block4 / block5 launch, forward and backward].  64 x 64 tiles (4 waves of
  // 32 x 32) put 4x the workgroups on the chip and a k-step costs a quarter of the MFMAs.  Every output element still sees
  // the same chain of MFMAs in the same k order, so the results are bit-identical to the large tiles (batch invariance).
  // LRP_CONV_SMALL=0 disables.
  const bool small = s.conv_small && t.BM == 128 && t.BN >= 64 && grid <= CONV_SMALL_BLOCKS;
  if (q.up2_src) {
    // compact pool interface into a pipelined halo kernel (128 x 128 or 8-wave; LRP_UP2_PW=0 disables): the grid must be
    // one that takes such a kernel without the request, and the loader must fit (below)
    if (!mul || prec != PREC_BF16X3 || !s.up2_pw || mode <= 0 || t.BN < 128 || small || !conv_compact_shape(q.N, q.Cin, q.H, q.W))
      return refused;
  } else if (small) {
    t = {64, 64};
    p.m_tiles = (p.M + 63) / 64;
    p.n_tiles = (q.N + 63) / 64;
    return done(FORM_SMALL);
  } else if (s.conv_mid && s.conv_small && t.BM == 128 && t.BN == 128 && (q.N % 64) == 0 && grid <= 2 * CONV_SMALL_BLOCKS) {
    // In between (at most one large tile per CU, but too many for the 64 x 64 tiles to stay resident): 128 x 64 tiles put two
    // workgroups on a CU and halve a k-step — same chains, same bits [MI355X, one image, ten words: block4's walk launches
    // (252 large tiles) 115 -> ~80 us, explain 1.62 -> 1.51 ms].  LRP_CONV_MID=0 disables.
    t = {128, 64};
    p.n_tiles = (q.N + 63) / 64;
  }
  // N = 64 tiles (TM x TN = 2 x 1 per wave) lose with the resident image: 2 instead of 3 blocks per CU and the
  // per-tap address work is spread over half as many MFMAs  [MI355X: block1_conv2 bwd 4.5 ms vs 5.2 ms]
  if (mode > 0 && (t.BN >= 128 || (mode == 2 && t.BN >= 64 && !q.dual_mul)) && resident(false, 0.9f)) {
    // the loader of the compact pool interface handles two items per thread and channel chunk
    if (q.up2_src && p.hrows * ((p.tw + 2) / 2 + 1) * 4 > 2 * (t.BM == 256 ? 512 : 256)) return refused;
    // the 8-wave tile of the dense split-bf16 walk with a fragment-major weight copy: weights in registers, one barrier per
    // channel chunk instead of one per tap (LRP_CONV_BREG8=0 disables).  A launch that carries a request keeps the pipelined
    // kernel (its window loader is ordered by the tap barriers); so does the tail of a residual block (ConvArgs::join).
    if (t.BM == 256 && (frag & (1u << FORM_BREG8)) && !asked && !q.join) return done(FORM_BREG8);
    // the same loop on the 128 x 128 tile (LRP_CONV_BREG4=0 disables): the dense split-bf16 walk launches and the interleaved
    // fp16-pair dual forward, N a multiple of the tile.  The walk launch may read the compact pool interface (its window loader
    // is sequenced by the chunk's steps there, for resident images that span two images at most); img_part and pool_gc never get here.
    if (t.BM == 128 && t.BN == 128 && (frag & (1u << FORM_BREG4)) && (epi != EPI_FWD_DUAL || q.dual_il) && !q.join &&
        !(q.up2_src && p.hrows > q.H))
      return done(FORM_BREG4);
    return done(FORM_HALO);
  }
  if (asked) return refused;                             // only the resident-image kernels read the compact pool interface
  return done(FORM_PLAIN);
}

}  // namespace lrp
