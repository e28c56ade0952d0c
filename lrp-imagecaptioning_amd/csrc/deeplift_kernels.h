// deeplift_kernels.h — the streaming passes of the DeepLIFT walk (Encoder::dl_pass / explain_deeplift, lrp_op_deeplift_conv).
// Reference semantics: innvestigate DeepLIFT with LinearRule on every fused conv + ReLU layer (deeplift.py:77-115):
//   t   = dX * convT( M A / (dY + 1e-7 [dY == 0]) )     SafeDivide, layers.py:446-461
//   g   =      convT( M A )
//   out = |dX| < 1e-7 ? g : t                           approximate_gradient=True (False: out = t)
// with dX = X - Xr, dY = Y - Yr against ONE reference forward shared by all images, M the ReLU mask of the actual forward, and
// max-pools routed to the actual forward's arg-max.  The two transposed convs are the existing exact-fp32 launches over the
// chains stacked along the batch axis ([t rows ; g rows]); everything else is here.  All three kernels are memory-bound
// streaming passes: four channels (16 bytes) per thread and access, grid-stride, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_args.h"

namespace lrp {

// SafeDivide's denominator: d + 1e-7 where d == 0 (layers.py:446-461)
__device__ __forceinline__ float dl_safe(float d) { return d == 0.f ? 1e-7f : d; }

// The gate of one layer, once per image at encode:  D = M ? safe(Y - Yr) : 0  — the masked DENOMINATOR, not its reciprocal: the
// walk divides by it, one rounding as in the reference's A / safe(dY); safe() never returns 0, so D != 0 is the mask M itself.
//   no pool behind the layer (gmask == nullptr): Y = y (the layer's activation), M = [Y > 0]
//   pooled layer: M = [gmask != 0] — the forward's gate, non-zero at the window's first arg-max where the unit is alive — and
//                 Y = pooled[window] there; yr stays at FULL resolution (the reference has its own arg-max)
// yr: one image's worth (H, W, C), shared by the batch.
__global__ __launch_bounds__(256) void dl_gate_kernel(const float* __restrict__ y, const float* __restrict__ gmask, const float* __restrict__ pooled,
                                                      const float* __restrict__ yr, float* __restrict__ out, int NB, int H, int W, int C) {
  const int C4 = C >> 2;
  const size_t per4 = (size_t)H * W * C4, total = (size_t)NB * per4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t n = i / per4, e = i - n * per4;
    f32x4 v, m;
    if (gmask) {
      const int c4 = (int)(e % C4);
      size_t r = e / C4;
      const int w = (int)(r % W), h = (int)(r / W);
      m = *reinterpret_cast<const f32x4*>(gmask + i * 4);
      v = *reinterpret_cast<const f32x4*>(pooled + (((n * (H >> 1) + (h >> 1)) * (W >> 1) + (w >> 1)) * C) + 4 * c4);
    } else {
      v = *reinterpret_cast<const f32x4*>(y + i * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) m[c] = v[c] > 0.f ? 1.f : 0.f;
    }
    const f32x4 rv = *reinterpret_cast<const f32x4*>(yr + e * 4);
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = m[c] != 0.f ? dl_safe(v[c] - rv[c]) : 0.f;
    *reinterpret_cast<f32x4*>(out + i * 4) = o;
  }
}

// Between two transposed convs.  c holds what the conv through layer l returned for the n tokens' chains, (rows, H, W, C) with
// rows = 2n [t ; g] (TWO) or n (t alone); x / xr the kept input of layer l (per image / the reference's, (H, W, C)); dn the gate D of
// layer l - 1, at this resolution or — POOL — at twice it:
//   o     = TWO && |x - xr| < 1e-7 ? g : (x - xr) t           the select (deeplift.py:100-113)
//   t'    = dn != 0 ? o / dn : 0,   g' = dn != 0 ? o : 0      both gates of the layer below; POOL: at the window's four cells,
//                                                              of which dn is non-zero at the arg-max only (the 2x routing)
// x == nullptr: the head of a walk — c is the caller's tensor (n rows, no select), o = c.
// out: (rows, H', W', C), H' = 2H under POOL.
template <bool TWO, bool POOL>
__global__ __launch_bounds__(256) void dl_combine_kernel(const float* __restrict__ c, const float* __restrict__ x, const float* __restrict__ xr,
                                                         const float* __restrict__ dn, const int* __restrict__ row2img, float* __restrict__ out,
                                                         int n, int H, int W, int C) {
  const int C4 = C >> 2;
  const size_t per = (size_t)H * W * C, per4 = per >> 2, total = (size_t)n * per4;
  constexpr int UP = POOL ? 4 : 1;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t t = i / per4, e4 = i - t * per4, e = e4 * 4;
    const size_t img = row2img ? (size_t)row2img[t] : t;
    f32x4 o = *reinterpret_cast<const f32x4*>(c + t * per + e);
    if (x) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + img * per + e), xrv = *reinterpret_cast<const f32x4*>(xr + e);
      f32x4 gv = o;
      if constexpr (TWO) gv = *reinterpret_cast<const f32x4*>(c + ((size_t)n + t) * per + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dx = xv[k] - xrv[k];
        o[k] = (TWO && fabsf(dx) < 1e-7f) ? gv[k] : dx * o[k];
      }
    }
    size_t off[UP];
    if constexpr (POOL) {
      const int c4 = (int)(e4 % C4);
      const size_t r = e4 / C4;
      const int w = (int)(r % W), h = (int)(r / W);
#pragma unroll
      for (int p = 0; p < 4; ++p) off[p] = ((size_t)(2 * h + (p >> 1)) * (2 * W) + 2 * w + (p & 1)) * C + 4 * c4;
    } else {
      off[0] = e;
    }
    const size_t pern = per * UP;
#pragma unroll
    for (int p = 0; p < UP; ++p) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(dn + img * pern + off[p]);
      f32x4 ot, og;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ot[k] = d[k] != 0.f ? o[k] / d[k] : 0.f;
        og[k] = d[k] != 0.f ? o[k] : 0.f;
      }
      *reinterpret_cast<f32x4*>(out + t * pern + off[p]) = ot;
      if constexpr (TWO) *reinterpret_cast<f32x4*>(out + ((size_t)n + t) * pern + off[p]) = og;
    }
  }
}

// End of a walk (the image layer), and the operator's output: the select alone, V elements per thread (V = 4 where a map's
// element count is a multiple of 4, else 1: three-channel images of odd area).  c: (rows, per), x: (images, per), xr: (per).
template <bool TWO, int V>
__global__ __launch_bounds__(256) void dl_final_kernel(const float* __restrict__ c, const float* __restrict__ x, const float* __restrict__ xr,
                                                       const int* __restrict__ row2img, float* __restrict__ out, int n, size_t per) {
  const size_t perv = per / V, total = (size_t)n * perv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t t = i / perv, e = (i - t * perv) * V;
    const size_t img = row2img ? (size_t)row2img[t] : t;
    float tv[V], gv[V] = {}, xv[V], xrv[V], o[V];
    if constexpr (V == 4) {
      *reinterpret_cast<f32x4*>(tv) = *reinterpret_cast<const f32x4*>(c + t * per + e);
      if constexpr (TWO) *reinterpret_cast<f32x4*>(gv) = *reinterpret_cast<const f32x4*>(c + ((size_t)n + t) * per + e);
      *reinterpret_cast<f32x4*>(xv) = *reinterpret_cast<const f32x4*>(x + img * per + e);
      *reinterpret_cast<f32x4*>(xrv) = *reinterpret_cast<const f32x4*>(xr + e);
    } else {
      tv[0] = c[t * per + e];
      if constexpr (TWO) gv[0] = c[((size_t)n + t) * per + e];
      xv[0] = x[img * per + e];
      xrv[0] = xr[e];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float dx = xv[k] - xrv[k];
      o[k] = (TWO && fabsf(dx) < 1e-7f) ? gv[k] : dx * tv[k];
    }
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(out + t * per + e) = *reinterpret_cast<const f32x4*>(o);
    else out[t * per + e] = o[0];
  }
}

}  // namespace lrp
