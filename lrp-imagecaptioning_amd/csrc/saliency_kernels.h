// saliency_kernels.h — the two model-agnostic word saliencies: occlusion sensitivity (Zeiler & Fergus, ECCV 2014) and RISE
// (Petsiuk, Das & Saenko, BMVC 2018).  Neither reads a gradient or the model's structure: masked copies of the image go through
// the ordinary forward (lrp_encode_images, lrp_decoder_forward, lrp_perturb_word_scores) and the word scores are folded back
// into a map.  Streaming kernels in the style of augment_kernels.h / perturb_kernels.h: device pointers, no atomics, every output
// element written by exactly one thread in one fixed order, so a row (or a map) never depends on what else shares the launch.
//
//  Occlusion geometry: window (ph, pw), stride (sh, sw), 1 <= sh <= ph <= H and 1 <= sw <= pw <= W; Hn = ceil((H - ph) / sh) + 1
//  windows per column (Wn alike), window k = i * Wn + j covers rows [i sh, min(i sh + ph, H)) and columns [j sw, min(j sw + pw, W)):
//  the last window of an axis is clipped and every pixel is covered (sh <= ph leaves no gap).
//  occlude_kernel         row r = image img_idx[r] with window k[r] set to fill[c], every channel; k = -1 copies the image.  An
//                         image index outside [0, B) or a k outside [-1, Hn Wn) gives a NaN row (as perturb_apply_kernel does).
//  occlusion_map_kernel   scores (n_img, 1 + Hn Wn, T) fp64, row 0 the unoccluded score -> S[t][y][x] = (sum over the windows k
//                         that cover (y, x), ascending k, of s_0[t] - s_{1+k}[t]) / c(y, x) in fp64, rounded once; c = the number
//                         of covering windows.  A gather of at most ceil(ph / sh) ceil(pw / sw) terms per pixel.
//
//  RISE: mask k of an image is a random (s + 1)^2 grid of {0, 1} cells, each 1 with probability p, upsampled bilinearly by exactly
//  (ch, cw) pixels per cell about half-pixel centres and cropped at a random shift (dy, dx) in [0, ch) x [0, cw).
//  rise_grids_kernel      Philox4x32-10 of augment_kernels.h, key = (seed low word, seed high word).  Cell e = a (s + 1) + c takes
//                         lane e % 4 of counter (e / 4, k, key, 1): `key` is the caller's identity of the image (not its slot in a
//                         call), the last word 1 separates this stream from the Gaussian augment's (whose last word is 0).
//                         G = 1 iff (x >> 8) < T with T = floor(p 2^24) computed by the host in double (p = 1: all ones).  The
//                         shifts come from counter (0xFFFFFFFF, k, key, 1): dy = x0 % ch, dx = x1 % cw.  The modulo bias
//                         (at most ch / 2^32 relative) is accepted.
//  the mask at pixel (y, x), stated once (rise_mask below; tests/saliency_ref.py restates it in float64):
//                         Y = y + dy, ny = 2 Y + 1 - ch, a0 = floor_div(ny, 2 ch), fy = (ny - 2 ch a0) / (2 ch); the rows a0 and
//                         a0 + 1 are clamped into [0, s]; columns alike from x + dx and cw; with top = G[a0][c0] + fx (G[a0][c1] -
//                         G[a0][c0]) and bot alike on row a1, m = top + fy (bot - top).
//                         Deviation from the paper: RISE draws an s x s grid and resizes it by the non-integer factor
//                         (s + 1) ceil(H / s) / s; here the grid has (s + 1)^2 cells and the factor is the integer (ch, cw), so a
//                         mask is an exact function of integers.  Away from the clamped border the two agree in distribution.
//  rise_apply_kernel      out = fill + m (x - fill) in float32, each operation rounded on its own (m: at most six roundings).  A
//                         row whose image index is outside [0, B) or whose shift is outside [0, ch) x [0, cw) comes out as NaN.
//  rise_map_kernel        scores (n_img, K, T) fp64 -> S[t][y][x] = (sum over k ascending of s_k[t] m_k(y, x)) / (K p), the masks
//                         recomputed in fp64 from the grids (no (K, H, W) tensor exists).  One thread per pixel and tile of
//                         RISE_TT words adds its K terms in ascending k: the order depends on nothing but K.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "augment_kernels.h"

namespace lrp {

constexpr int OCC_MAX_WINDOWS = 65536;
constexpr int RISE_MAX_S = 63;
constexpr int RISE_MAX_CELL = 1 << 20;     // 2 (y + dy) + 1 stays far inside int32
constexpr int RISE_TT = 8;                 // words per thread of rise_map_kernel (saliency.py pads T to it: _TILE)

struct OccGeom {
  int H, W, C;
  int ph, pw, sh, sw;
  int Hn, Wn;
};

struct RiseGeom {
  int H, W, C;
  int s, ch, cw;
};

__device__ __forceinline__ float sal_nan() { return __int_as_float(0x7fc00000); }

__device__ __forceinline__ int sal_floor_div(int a, int b) {      // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// VEC: per_image % 4 == 0 and 16-byte aligned bases: a group is one float4; otherwise up to four scalar accesses (a tail group of
// a row holds fewer than four values)
template <bool VEC>
__global__ __launch_bounds__(256) void occlude_kernel(const float* __restrict__ x, const int* __restrict__ img_idx,
                                                      const int* __restrict__ kk, const float* __restrict__ fill,
                                                      float* __restrict__ out, int n, int B, OccGeom g) {
  const size_t per = (size_t)g.H * g.W * g.C, groups = (per + 3) / 4, total = (size_t)n * groups;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t rr = idx / groups, gi = idx - rr * groups;
    const int e0 = (int)(4 * gi);
    const int lim = per - e0 < 4 ? (int)(per - e0) : 4;
    float* dst = out + rr * per + e0;
    const int img = img_idx[rr], k = kk[rr];
    float v[4];
    if (img < 0 || img >= B || k < -1 || k >= g.Hn * g.Wn) {
      v[0] = v[1] = v[2] = v[3] = sal_nan();
    } else {
      const float* src = x + (size_t)img * per + e0;
      if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        for (int e = 0; e < lim; ++e) v[e] = src[e];
      }
      if (k >= 0) {
        const int wi = k / g.Wn, wj = k - wi * g.Wn;
        const int y0 = wi * g.sh, x0 = wj * g.sw, y1 = y0 + g.ph, x1 = x0 + g.pw;     // (rows / columns past the image do not exist)
        int p = e0 / g.C, c = e0 - p * g.C, y = p / g.W, xx = p - y * g.W;
        for (int e = 0; e < lim; ++e) {
          if (y >= y0 && y < y1 && xx >= x0 && xx < x1) v[e] = fill[c];
          if (++c == g.C) { c = 0; if (++xx == g.W) { xx = 0; ++y; } }
        }
      }
    }
    if (VEC) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int e = 0; e < lim; ++e) dst[e] = v[e];
    }
  }
}

__global__ __launch_bounds__(256) void occlusion_map_kernel(const double* __restrict__ scores, float* __restrict__ out, int n_img,
                                                            int T, OccGeom g) {
  const size_t hw = (size_t)g.H * g.W, total = (size_t)n_img * T * hw;
  const size_t nrow = 1 + (size_t)g.Hn * g.Wn;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t it = idx / hw;
    const int p = (int)(idx - it * hw), y = p / g.W, xx = p - y * g.W;
    const size_t img = it / T;
    const int t = (int)(it - img * T);
    const double* sc = scores + img * nrow * T + t;
    const int i_lo = y - g.ph + 1 <= 0 ? 0 : (y - g.ph + g.sh) / g.sh, i_hi = min(g.Hn - 1, y / g.sh);
    const int j_lo = xx - g.pw + 1 <= 0 ? 0 : (xx - g.pw + g.sw) / g.sw, j_hi = min(g.Wn - 1, xx / g.sw);
    const double s0 = sc[0];
    double acc = 0.0;
    for (int i = i_lo; i <= i_hi; ++i)
      for (int j = j_lo; j <= j_hi; ++j) acc += s0 - sc[(size_t)(1 + i * g.Wn + j) * T];
    const int cnt = (i_hi - i_lo + 1) * (j_hi - j_lo + 1);          // >= 1: every pixel is covered
    out[idx] = (float)(acc / (double)cnt);
  }
}

// one thread per (row, group of four cells); the thread past a row's last group draws the row's shift
__global__ __launch_bounds__(256) void rise_grids_kernel(const unsigned* __restrict__ key, const int* __restrict__ kk, int n, int s,
                                                         unsigned thresh, unsigned seed_lo, unsigned seed_hi, int ch, int cw,
                                                         unsigned char* __restrict__ grid, int* __restrict__ shift) {
  const int cells = (s + 1) * (s + 1), groups = (cells + 3) / 4;
  const size_t total = (size_t)n * (groups + 1);
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t rr = idx / (groups + 1);
    const int gi = (int)(idx - rr * (groups + 1));
    const unsigned k = (unsigned)kk[rr], id = key[rr];
    if (gi == groups) {
      const Philox4 r = philox4x32_10(0xFFFFFFFFu, k, id, 1u, seed_lo, seed_hi);
      shift[2 * rr] = (int)(r.v[0] % (unsigned)ch);
      shift[2 * rr + 1] = (int)(r.v[1] % (unsigned)cw);
    } else {
      const Philox4 r = philox4x32_10((unsigned)gi, k, id, 1u, seed_lo, seed_hi);
      unsigned char* dst = grid + rr * cells + 4 * gi;
      const int lim = cells - 4 * gi < 4 ? cells - 4 * gi : 4;
      for (int e = 0; e < lim; ++e) dst[e] = (r.v[e] >> 8) < thresh ? 1 : 0;
    }
  }
}

// The mask of one pixel (see the header of this file), in F = float (the apply kernel: every operation rounded on its own) or
// double (the map kernel).  G: the (s + 1)^2 cells of one mask.
template <typename F>
__device__ __forceinline__ void rise_axis(int pos, int cell, int s, int& a0, int& a1, F& f) {
  const int nn = 2 * pos + 1 - cell, q = sal_floor_div(nn, 2 * cell);
  f = (F)(nn - 2 * cell * q) / (F)(2 * cell);
  a0 = min(max(q, 0), s);
  a1 = min(max(q + 1, 0), s);
}

__device__ __forceinline__ float rise_lerp(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(f, __fsub_rn(b, a))); }
__device__ __forceinline__ double rise_lerp(double a, double b, double f) { return __dadd_rn(a, __dmul_rn(f, __dsub_rn(b, a))); }

template <typename F>
__device__ __forceinline__ F rise_mask(const unsigned char* __restrict__ G, int s, int a0, int a1, F fy, int c0, int c1, F fx) {
  const F g00 = G[a0 * (s + 1) + c0] ? (F)1 : (F)0, g01 = G[a0 * (s + 1) + c1] ? (F)1 : (F)0;
  const F g10 = G[a1 * (s + 1) + c0] ? (F)1 : (F)0, g11 = G[a1 * (s + 1) + c1] ? (F)1 : (F)0;
  return rise_lerp(rise_lerp(g00, g01, fx), rise_lerp(g10, g11, fx), fy);
}

template <bool VEC>
__global__ __launch_bounds__(256) void rise_apply_kernel(const float* __restrict__ x, const int* __restrict__ img_idx,
                                                         const unsigned char* __restrict__ grid, const int* __restrict__ shift,
                                                         const float* __restrict__ fill, float* __restrict__ out, int n, int B,
                                                         RiseGeom g) {
  const size_t per = (size_t)g.H * g.W * g.C, groups = (per + 3) / 4, total = (size_t)n * groups;
  const int cells = (g.s + 1) * (g.s + 1);
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t rr = idx / groups, gi = idx - rr * groups;
    const int e0 = (int)(4 * gi);
    const int lim = per - e0 < 4 ? (int)(per - e0) : 4;
    float* dst = out + rr * per + e0;
    const int img = img_idx[rr], dy = shift[2 * rr], dx = shift[2 * rr + 1];
    float v[4];
    if (img < 0 || img >= B || dy < 0 || dy >= g.ch || dx < 0 || dx >= g.cw) {
      v[0] = v[1] = v[2] = v[3] = sal_nan();
    } else {
      const float* src = x + (size_t)img * per + e0;
      if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        for (int e = 0; e < lim; ++e) v[e] = src[e];
      }
      const unsigned char* G = grid + rr * cells;
      int p = e0 / g.C, c = e0 - p * g.C, y = p / g.W, xx = p - y * g.W;
      int a0, a1, c0, c1;
      float fy, fx, m = 0.f;
      bool fresh = true;                                             // the pixel changed: its mask is computed once
      for (int e = 0; e < lim; ++e) {
        if (fresh) {
          rise_axis<float>(y + dy, g.ch, g.s, a0, a1, fy);
          rise_axis<float>(xx + dx, g.cw, g.s, c0, c1, fx);
          m = rise_mask<float>(G, g.s, a0, a1, fy, c0, c1, fx);
        }
        const float f = fill[c];
        v[e] = __fadd_rn(f, __fmul_rn(m, __fsub_rn(v[e], f)));
        fresh = false;
        if (++c == g.C) { c = 0; fresh = true; if (++xx == g.W) { xx = 0; ++y; } }
      }
    }
    if (VEC) {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int e = 0; e < lim; ++e) dst[e] = v[e];
    }
  }
}

// block = (image, tile of RISE_TT words, 256 pixels); scores / shifts are read at wave-uniform addresses, the four cells of a
// mask from its (s + 1)^2 bytes.  A shift outside [0, ch) x [0, cw) makes the term NaN (nothing outside the grid is read).
__global__ __launch_bounds__(256) void rise_map_kernel(const double* __restrict__ scores, const unsigned char* __restrict__ grid,
                                                       const int* __restrict__ shift, float* __restrict__ out, int K, int T,
                                                       RiseGeom g, double denom) {
  const int hw = g.H * g.W, pb = (hw + 255) / 256, tiles = (T + RISE_TT - 1) / RISE_TT;
  const int blk = blockIdx.x;
  const int pblk = blk % pb, tile = (blk / pb) % tiles;
  const size_t img = (size_t)(blk / pb / tiles);
  const int p = pblk * 256 + threadIdx.x;
  if (p >= hw) return;
  const int y = p / g.W, xx = p - y * g.W, t0 = tile * RISE_TT, nt = min(RISE_TT, T - t0);
  const int cells = (g.s + 1) * (g.s + 1);
  const double* sc = scores + img * (size_t)K * T + t0;
  const unsigned char* G = grid + img * (size_t)K * cells;
  const int* sh = shift + img * (size_t)K * 2;
  double acc[RISE_TT];
#pragma unroll
  for (int j = 0; j < RISE_TT; ++j) acc[j] = 0.0;
  for (int k = 0; k < K; ++k, sc += T, G += cells, sh += 2) {
    const int dy = sh[0], dx = sh[1];
    double m;
    if (dy < 0 || dy >= g.ch || dx < 0 || dx >= g.cw) {
      m = 0.0 / 0.0;
    } else {
      int a0, a1, c0, c1;
      double fy, fx;
      rise_axis<double>(y + dy, g.ch, g.s, a0, a1, fy);
      rise_axis<double>(xx + dx, g.cw, g.s, c0, c1, fx);
      m = rise_mask<double>(G, g.s, a0, a1, fy, c0, c1, fx);
    }
#pragma unroll
    for (int j = 0; j < RISE_TT; ++j)
      if (j < nt) acc[j] = __dadd_rn(acc[j], __dmul_rn(sc[j], m));
  }
#pragma unroll
  for (int j = 0; j < RISE_TT; ++j)
    if (j < nt) out[(img * T + t0 + j) * (size_t)hw + p] = (float)(acc[j] / denom);
}

}  // namespace lrp
