// conv_launch.h — the host launchers of conv_igemm_kernel: they execute the plan of conv_plan.h.
#pragma once
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"
#include "conv_igemm.h"
#include "conv_plan.h"

namespace lrp {

// device table of a.order for this call's token -> image map (see TileOrder); nullptr when the stack order is as good
inline const int* conv_tile_order(const ConvArgs& a, hipStream_t st) {
  if (!sw().tile_order || !a.order || !a.row2img_host || a.NB < 2 || a.th < 1) return nullptr;
  TileOrder& o = *a.order;
  const int tiles_y = a.tpt > 0 ? a.NB * a.tpt : (a.nyh + a.th - 1) / a.th;
  const bool same = o.H == a.H && o.th == a.th && o.nyh == a.nyh && o.cols_t == a.cols_t && o.tpt == a.tpt && (int)o.sig.size() == a.NB &&
                    memcmp(o.sig.data(), a.row2img_host, (size_t)a.NB * sizeof(int)) == 0;
  if (same) return o.identity ? nullptr : o.dev;
  o.sig.assign(a.row2img_host, a.row2img_host + a.NB);
  o.H = a.H; o.th = a.th; o.nyh = a.nyh; o.cols_t = a.cols_t; o.tpt = a.tpt;
  constexpr int band = 1, strip = 2;                   // row band of `band` tile rows per token; column tiles per strip (measured, round 2)
  std::vector<long long> key((size_t)tiles_y);
  for (int ty = 0; ty < tiles_y; ++ty) {
    int Ym = a.tpt > 0 ? (ty / a.tpt) * a.H + (ty % a.tpt) * a.th + a.th / 2 : ty * a.th + a.th / 2;
    if (a.tpt > 0 && Ym > (ty / a.tpt + 1) * a.H - 1) Ym = (ty / a.tpt + 1) * a.H - 1;
    if (Ym > a.nyh - 1) Ym = a.nyh - 1;
    const int t = Ym / a.H, hpos = Ym - t * a.H;
    key[ty] = ((long long)o.sig[t] << 42) | ((long long)(hpos / (a.th * band)) << 21) | (long long)t;
  }
  std::vector<int> rows((size_t)tiles_y);
  for (int i = 0; i < tiles_y; ++i) rows[i] = i;
  std::stable_sort(rows.begin(), rows.end(), [&](int x, int y) { return key[x] < key[y]; });
  // rows are now (image, band, token); within an image, walk the column strips outermost
  const int sw = strip > 0 && strip < a.cols_t ? strip : a.cols_t;
  const size_t m_tiles = (size_t)tiles_y * a.cols_t;
  std::vector<int> map;
  map.reserve(m_tiles);
  for (int r0 = 0; r0 < tiles_y;) {
    int r1 = r0;
    while (r1 < tiles_y && (key[rows[r1]] >> 42) == (key[rows[r0]] >> 42)) ++r1;
    for (int c0 = 0; c0 < a.cols_t; c0 += sw)
      for (int r = r0; r < r1; ++r)
        for (int c = c0; c < c0 + sw && c < a.cols_t; ++c) map.push_back(rows[r] * a.cols_t + c);
    r0 = r1;
  }
  o.identity = true;
  for (size_t i = 0; i < m_tiles; ++i)
    if (map[i] != (int)i) { o.identity = false; break; }
  if (o.identity) return nullptr;
  if (o.ev) (void)hipEventSynchronize(o.ev);            // the staging buffer may still feed the previous upload
  if (o.cap < m_tiles) {
    if (o.dev) (void)hipFree(o.dev);
    if (o.pinned) (void)hipHostFree(o.pinned);
    o.dev = o.pinned = nullptr;
    o.cap = 0;
    if (hipMalloc((void**)&o.dev, m_tiles * sizeof(int)) != hipSuccess ||
        hipHostMalloc((void**)&o.pinned, m_tiles * sizeof(int), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      o.sig.clear();                                    // (try again next call; this one runs in stack order)
      return nullptr;
    }
    o.cap = m_tiles;
  }
  memcpy(o.pinned, map.data(), m_tiles * sizeof(int));
  if (!o.ev) (void)hipEventCreateWithFlags(&o.ev, hipEventDisableTiming);
  if (hipMemcpyAsync(o.dev, o.pinned, m_tiles * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) {
    (void)hipGetLastError();
    o.sig.clear();
    return nullptr;
  }
  (void)hipEventRecord(o.ev, st);
  return o.dev;
}

// the question conv_plan is asked about the launch of `a`
inline ConvAsk conv_ask(int epi, int prec, int terms, bool gmask, const ConvArgs& a) {
  ConvAsk q;
  q.epi = epi; q.prec = prec; q.terms = terms; q.gmask = gmask;
  q.NB = a.NB; q.H = a.H; q.W = a.W; q.N = a.N; q.Cin = a.Cin; q.taps = a.taps;
  q.frag = a.wpk_frag != nullptr; q.join = a.join != nullptr; q.dual_il = a.dual_il != 0; q.split = a.split;
  q.up2_src = a.up2_src != nullptr; q.img_part = a.img_part != nullptr; q.pool_gc = a.pool_gc != nullptr;
  q.dual_mul = a.out_b != nullptr;
  return q;
}
inline void conv_apply_plan(const ConvPlan& p, ConvArgs& a) {
  a.M = p.M; a.m_tiles = p.m_tiles; a.n_tiles = p.n_tiles;
  a.tw = p.tw; a.th = p.th; a.hrows = p.hrows; a.cols_t = p.cols_t; a.nyh = p.nyh; a.tpt = p.tpt;
  a.epi_generic = p.epi_generic;
}

// EPI_IMG_STENCIL: NB = image slots (tokens), H x W = the image; in = S_1 (NB, H, W, Cin); N = 54 <= 64
template <int PREC>
inline hipError_t conv_launch_img(ConvArgs a, hipStream_t st) {
  if (!a.ximg || (PREC == PREC_F16X2 && !a.tok_fac)) return hipErrorInvalidValue;
  const ConvPlan p = conv_plan(conv_ask(EPI_IMG_STENCIL, PREC, 7, false, a));
  if (!p.ok) return hipErrorInvalidValue;
  if (a.NB <= 0) return hipSuccess;
  conv_apply_plan(p, a);
  a.tiles_x = (a.W + IMG_TILE - 1) / IMG_TILE;
  a.tiles_y = (a.H + IMG_TILE - 1) / IMG_TILE;
  hipLaunchKernelGGL((conv_igemm_kernel<4, 1, 2, 2, EPI_IMG_STENCIL, PREC>), dim3(a.m_tiles), dim3(p.threads), 0, st, a);
  return hipGetLastError();
}

// one arm of conv_launch_epi: entry I of CONV_FORM_TILES, compiled only where this (EPI, PREC, TERMS, GMASK, DG) has a kernel on it
// FORM_BREG has two loops, and which one a launch runs on is decided here, not in the plan: the chunk loop where it exists (the
// dense split-bf16 walk) unless LRP_CONV_BREG2=0; on it, a launch that reads the compact pool interface takes the PW instantiation.
template <int I, int EPI, int PREC, int TERMS, bool GMASK, bool DG>
inline bool conv_launch_form(const ConvPlan& p, ConvArgs& a, hipStream_t st) {
  constexpr ConvFormTile F = CONV_FORM_TILES[I];
  if constexpr (conv_kernel_exists(F.form, F.BM, F.BN, F.pw, EPI, PREC, TERMS, GMASK, DG, F.c2)) {
    const bool c2 = p.form == FORM_BREG && sw().conv_breg2 && conv_kernel_exists(FORM_BREG, 128, 64, false, EPI, PREC, TERMS, GMASK, DG, true);
    const bool pw = p.pw || (c2 && a.up2_src);
    if (p.form != F.form || p.BM != F.BM || p.BN != F.BN || pw != F.pw || c2 != F.c2) return false;
    constexpr ConvKernelShape K = conv_kernel_shape(F.form, F.BM, F.BN, F.pw, F.c2);
    if (K.HALO && (EPI == EPI_MUL || EPI == EPI_MUL_UP2)) a.tile_map = conv_tile_order(a, st);
    hipLaunchKernelGGL((conv_igemm_kernel<K.WM, K.WN, K.TM, K.TN, EPI, PREC, K.HALO, K.BREG, TERMS, K.NS, GMASK, K.PW, DG, K.C2>),
                       dim3(p.m_tiles * p.n_tiles), dim3(p.threads), 0, st, a);
    return true;
  }
  return false;
}
template <int EPI, int PREC, int TERMS, bool GMASK, bool DG, int... I>
inline bool conv_launch_forms(const ConvPlan& p, ConvArgs& a, hipStream_t st, std::integer_sequence<int, I...>) {
  return (conv_launch_form<I, EPI, PREC, TERMS, GMASK, DG>(p, a, st) || ...);
}

template <int EPI, int PREC, int TERMS = 7, bool GMASK = false, bool DG = false>
inline hipError_t conv_launch_epi(ConvArgs a, hipStream_t st) {
  static_assert(EPI != EPI_IMG_STENCIL && conv_epi_exists(EPI, PREC, TERMS, GMASK, DG), "conv_plan.h: no kernel has this epilogue in this format");
  constexpr bool MUL = EPI == EPI_MUL || EPI == EPI_MUL_UP2, FWD = EPI == EPI_BIAS || EPI == EPI_BIAS_RELU || EPI == EPI_FWD_DUAL;
  // 1. what only the pointers tell
  if (DG != (a.out_b != nullptr)) return hipErrorInvalidValue;
  if (DG && (!a.aux || !a.aux_b || !a.out || a.ostride < a.N || (a.ostride & (PREC != PREC_FP32 ? 7 : 3)) || a.out2s || a.gate_none ||
             a.gate_binary || a.relu_out))
    return hipErrorInvalidValue;
  if (GMASK && (a.out2s || a.gate_none)) return hipErrorInvalidValue;
  if (PREC == PREC_F16X2 && MUL && (!a.tok_fac || !a.tok_max_out || a.out_plain)) return hipErrorInvalidValue;
  if (PREC == PREC_F16X2 && FWD && !a.in_unscale) return hipErrorInvalidValue;
  // 2. the plan
  const ConvPlan p = conv_plan(conv_ask(EPI, PREC, TERMS, GMASK, a));
  if (!p.ok) return hipErrorInvalidValue;
  if (p.M <= 0 || a.N <= 0) return hipSuccess;
  // (what a request needs besides the form: only a launch that does something is held to it)
  if (a.pool_gc && (!a.pairs_out || !a.pool_pos)) return hipErrorInvalidValue;
  if (a.img_part && !a.img_w) return hipErrorInvalidValue;
  if (a.up2_src && (!a.up2_pairs || !a.up2_gpos)) return hipErrorInvalidValue;
  conv_apply_plan(p, a);
  // 3. its kernel.  (The plan answers through the predicate the arms are compiled by: it cannot name a kernel they lack.)
  if (!conv_launch_forms<EPI, PREC, TERMS, GMASK, DG>(p, a, st, std::make_integer_sequence<int, CONV_FORM_TILE_COUNT>{})) return hipErrorInvalidValue;
  return hipGetLastError();
}

// Runtime (epilogue, format, terms, dual gate) -> the launcher's template arguments: case I of every combination of the four axes,
// compiled where conv_epi_exists says it has kernels.  Everything else is hipErrorInvalidValue.
template <int I>
inline bool conv_launch_case(int epi, int prec, int terms, bool dual, const ConvArgs& a, hipStream_t st, hipError_t& e) {
  constexpr int EPI = I / 18, PREC = I / 6 % 3, TERMS = CONV_TERMS[I / 2 % 3];
  constexpr bool DG = I % 2;
  if constexpr (conv_epi_exists(EPI, PREC, TERMS, false, DG)) {
    if (epi != EPI || prec != PREC || terms != TERMS || dual != DG) return false;
    if constexpr (EPI == EPI_IMG_STENCIL) e = conv_launch_img<PREC>(a, st);
    else e = conv_launch_epi<EPI, PREC, TERMS, false, DG>(a, st);
    return true;
  }
  return false;
}
template <int... I>
inline hipError_t conv_launch_cases(int epi, int prec, int terms, bool dual, const ConvArgs& a, hipStream_t st, std::integer_sequence<int, I...>) {
  hipError_t e = hipErrorInvalidValue;
  (void)(conv_launch_case<I>(epi, prec, terms, dual, a, st, e) || ...);
  return e;
}
inline hipError_t conv_launch(int epi, const ConvArgs& a, hipStream_t st, int prec = PREC_FP32, int terms = 7) {
  const bool dual = a.out_b != nullptr;                // dual gate (ConvArgs::aux_b)
  return conv_launch_cases(epi, prec, conv_terms(prec, terms, dual), dual, a, st, std::make_integer_sequence<int, (EPI_IMG_STENCIL + 1) * 3 * 3 * 2>{});
}

// the ResNet gradient walks' transposed convs: exact fp32, `aux` / `join_gate` are byte masks (conv_igemm_kernel GMASK)
inline hipError_t conv_launch_grad_mask(const ConvArgs& a, hipStream_t st) {
  return conv_launch_epi<EPI_MUL, PREC_FP32, 7, true>(a, st);
}

}  // namespace lrp
