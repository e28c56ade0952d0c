// pattern_kernels.h — PatternNet / PatternAttribution for the VGG-style encoders (Encoder::pattern_*):
// innvestigate/tools/pattern.py (the fit) and analyzer/pattern_based.py (the walk), exact fp32.
//
// Fit, per conv and encoded batch: c = conv(x) + b without the ReLU; pattern_mask_kernel turns it into the two right-hand sides
// mask and (c - b) * mask of the products X^T . mask and X^T . (Y * mask) (train_gemm.h, the weight gradient's gathered taps) and
// into per-channel partial sums of Y = c - b and of mask; pattern_accumulate_kernel adds the batch to float64 sums;
// pattern_compute_kernel turns the sums into the pattern A = cov / safe(sum_k W * cov), one workgroup per output channel.
//
// Walk, per layer: the gradient walk's transposed conv over a packed copy of A (or A * W) with a plain accumulator out, the row's
// absolute maximum (partials in chunk order, then one thread per row), and pattern_project_kernel: the true division by that
// maximum, the ReLU mask of the layer below and the 2x2 pool's routing, written where the next conv reads.
//
// Order of every reduction: fixed by the shapes alone, no atomic.  A row's maximum does not depend on the order at all.
#pragma once
#include "cnn_kernels.h"
#include "common.h"

namespace lrp {

enum { PAT_LINEAR = 0, PAT_RELU_POSITIVE = 1, PAT_RELU_NEGATIVE = 2 };

constexpr int PAT_ITEMS_PER_BLOCK = 256 * 8;             // items (float4, or floats of a row that is no multiple of 4) per block
constexpr int PAT_MAX_CHUNKS = 2048;                    // position chunks of the mask pass

// ---- fit ------------------------------------------------------------------------------------------------------------------
// The image layer's pre-activation (cin = 3, K = 27): one thread per pixel and 4 output channels, products in tap order.
// w_fwd: the layer's forward matrix [.][64], row co holds w[k][co] at column k = tap * 3 + ci (pack_image_layer_dev_kernel).
// Dynamic LDS: 27 * cout floats.
__global__ __launch_bounds__(256) void pattern_image_conv_kernel(const float* __restrict__ x, const float* __restrict__ w_fwd,
                                                                 const float* __restrict__ bias, float* __restrict__ c, int NB, int H,
                                                                 int W, int cout) {
  extern __shared__ float pat_wl[];                      // [27][cout]
  for (int i = threadIdx.x; i < 27 * cout; i += 256) {
    const int k = i / cout, co = i - k * cout;
    pat_wl[i] = w_fwd[(size_t)co * 64 + k];
  }
  __syncthreads();
  const int cg = cout / 4;
  const size_t total = (size_t)NB * H * W * cg;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t pix = i / cg;
    const int c4 = (int)(i - pix * cg) * 4;
    const int xw = (int)(pix % W);
    const size_t r = pix / W;
    const int y = (int)(r % H);
    const size_t n = r / H;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < 9; ++t) {
      const int yy = y + t / 3 - 1, xx = xw + t % 3 - 1;
      if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
      const float* px = x + ((n * H + yy) * W + xx) * 3;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        const float xv = px[ci];
        const f32x4 wv = *reinterpret_cast<const f32x4*>(pat_wl + (t * 3 + ci) * cout + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(xv, wv[e], acc[e]);
      }
    }
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias + c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += b[e];
    *reinterpret_cast<f32x4*>(c + pix * cout + c4) = acc;
  }
}

// c (P, cout) -> m = mask, ym = (c - b) * mask (both (P, cout)); part [chunk][2 cout] float64: per channel the chunk's sum of
// c - b over ALL its positions, then the chunk's count of mask.  A block takes rows_per consecutive positions; a thread owns 4
// channels and every lanes-th position, adds them in ascending order, and the threads of a channel group are folded in lane order.
__global__ __launch_bounds__(256) void pattern_mask_kernel(const float* __restrict__ c, const float* __restrict__ bias,
                                                           float* __restrict__ m, float* __restrict__ ym, double* __restrict__ part,
                                                           long P, int cout, long rows_per, int type) {
  __shared__ double red[256][8];
  const int cg = cout / 4, cw = cg < 256 ? cg : 256, lanes = 256 / cw, tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * rows_per;
  const long r1 = r0 + rows_per < P ? r0 + rows_per : P;
  for (int g0 = 0; g0 < cg; g0 += cw) {
    const int gl = tid % cw, rl = tid / cw, g = g0 + gl;
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (rl < lanes && g < cg) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(bias + 4 * g);
      for (long r = r0 + rl; r < r1; r += lanes) {
        const size_t o = (size_t)r * cout + 4 * g;
        const f32x4 cv = *reinterpret_cast<const f32x4*>(c + o);
        f32x4 mv, yv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y = cv[e] - b[e];
          const bool on = type == PAT_LINEAR ? true : type == PAT_RELU_POSITIVE ? cv[e] > 0.f : cv[e] <= 0.f;
          mv[e] = on ? 1.f : 0.f;
          yv[e] = on ? y : 0.f;
          s[e] += (double)y;
          s[4 + e] += on ? 1.0 : 0.0;
        }
        *reinterpret_cast<f32x4*>(m + o) = mv;
        *reinterpret_cast<f32x4*>(ym + o) = yv;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid][e] = s[e];
    __syncthreads();
    if (rl == 0 && g < cg) {
      for (int j = 1; j < lanes; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += red[j * cw + gl][e];
      double* p = part + (size_t)blockIdx.x * 2 * cout;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[4 * g + e] = s[e];
        p[cout + 4 * g + e] = s[4 + e];
      }
    }
    __syncthreads();
  }
}

// sums: float64 [Sx (K cout) | Sxy (K cout) | cnt (cout) | Sy (cout) | P (1)].  prod: the batch's two products [Sx | Sxy] in fp32;
// part: pattern_mask_kernel's partials, folded in chunk order.
__global__ __launch_bounds__(256) void pattern_accumulate_kernel(const float* __restrict__ prod, const double* __restrict__ part,
                                                                 int chunks, double* __restrict__ sums, size_t KC, int cout,
                                                                 double positions) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t i = gid; i < 2 * KC; i += stride) sums[i] += (double)prod[i];
  for (size_t j = gid; j < (size_t)2 * cout; j += stride) {
    double s = 0.0;
    for (int q = 0; q < chunks; ++q) s += part[(size_t)q * 2 * cout + j];
    const size_t ch = j % cout;
    // (the partials hold [sum of y | count]; the sums hold [count | sum of y])
    sums[2 * KC + (j < (size_t)cout ? (size_t)cout : 0) + ch] += s;
  }
  if (gid == 0) sums[2 * KC + 2 * (size_t)cout] += positions;
}

// A[k][c] = cov[k][c] / safe(sum_k W[k][c] cov[k][c]),  cov = Sxy / safe(cnt) - Sx / safe(cnt) * (Sy / P),  safe(v) = v + [v == 0]:
// float64, one workgroup per output channel c; a thread adds its k = tid, tid + 256, ... in that order, the wave folds with a xor
// butterfly, thread 0 folds the waves in wave order.  W is read from the layer's packed forward matrix: row c, column
// tap * CP + ci (CP = 0: the image layer's [.][64] matrix, column k).  A: HWIO, float32.
__global__ __launch_bounds__(256) void pattern_compute_kernel(const double* __restrict__ sums, const float* __restrict__ wpk, int wrow,
                                                              int CP, int cin, int cout, float* __restrict__ A) {
  __shared__ double lds[5];
  const int c = blockIdx.x, K = 9 * cin, tid = threadIdx.x;
  const size_t KC = (size_t)K * cout;
  const double cnt = sums[2 * KC + c], sy = sums[2 * KC + cout + c], P = sums[2 * KC + 2 * (size_t)cout];
  const double sc = cnt + (cnt == 0.0 ? 1.0 : 0.0), my = sy / (P + (P == 0.0 ? 1.0 : 0.0));
  auto cov_at = [&](int k) { return sums[KC + (size_t)k * cout + c] / sc - sums[(size_t)k * cout + c] / sc * my; };
  double d = 0.0;
  for (int k = tid; k < K; k += 256) {
    const int t = k / cin, ci = k - t * cin;
    const double w = (double)(CP ? wpk[(size_t)c * wrow + t * CP + ci] : wpk[(size_t)c * wrow + k]);
    d += w * cov_at(k);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
  if ((tid & 63) == 0) lds[tid >> 6] = d;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) d += lds[w];
    lds[4] = d + (d == 0.0 ? 1.0 : 0.0);
  }
  __syncthreads();
  const double den = lds[4];
  for (int k = tid; k < K; k += 256) A[(size_t)k * cout + c] = (float)(cov_at(k) / den);
}

// ---- the walk's matrices ----------------------------------------------------------------------------------------------------
// the image layer's pattern (3,3,3,cout) HWIO -> the gradient walks' layout of that layer (pack_image_layer_dev_kernel's `full`)
__global__ __launch_bounds__(256) void pattern_pack_image_kernel(const float* __restrict__ A, float* __restrict__ full, int cout, int Kb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 27 * cout) return;
  const int k = i / cout, co = i - k * cout, t = k / 3, c = k - 3 * t;
  full[(size_t)(t * 6 + c) * Kb + co] = A[i];
}
// PatternAttribution: the packed pattern times the packed weights, element by element (same layout, padding stays zero)
__global__ __launch_bounds__(256) void pattern_mul_kernel(const f32x4* __restrict__ a, const f32x4* __restrict__ w, f32x4* __restrict__ out,
                                                          size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 av = a[i], wv = w[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = av[e] * wv[e];
    out[i] = o;
  }
}

// ---- walk -------------------------------------------------------------------------------------------------------------------
inline int pattern_chunks(size_t per_row) {
  const size_t items = (per_row & 3) ? per_row : per_row / 4;
  return (int)((items + PAT_ITEMS_PER_BLOCK - 1) / PAT_ITEMS_PER_BLOCK);
}
// grid (chunks, n): part[row][chunk] = max |x| over the chunk's items of the row (NaN is skipped)
__global__ __launch_bounds__(256) void pattern_absmax_part_kernel(const float* __restrict__ x, size_t per_row, float* __restrict__ part) {
  __shared__ float lds[4];
  const int row = blockIdx.y, tid = threadIdx.x;
  const float* r = x + (size_t)row * per_row;
  float mx = 0.f;
  if (!(per_row & 3)) {
    const size_t n4 = per_row / 4;
    for (int j = 0; j < 8; ++j) {
      const size_t it = (size_t)blockIdx.x * PAT_ITEMS_PER_BLOCK + (size_t)j * 256 + tid;
      if (it >= n4) break;
      const f32x4 v = reinterpret_cast<const f32x4*>(r)[it];
#pragma unroll
      for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fabsf(v[e]));
    }
  } else {
    for (int j = 0; j < 8; ++j) {
      const size_t it = (size_t)blockIdx.x * PAT_ITEMS_PER_BLOCK + (size_t)j * 256 + tid;
      if (it >= per_row) break;
      mx = fmaxf(mx, fabsf(r[it]));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) lds[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) mx = fmaxf(mx, lds[w]);
    part[(size_t)row * gridDim.x + blockIdx.x] = mx;
  }
}
// a row's partials in chunk order -> its divisor: the absolute maximum, 1 where that is 0 (layers.py:314-337).  One thread per row.
__global__ __launch_bounds__(64) void pattern_absmax_finish_kernel(const float* __restrict__ part, int n, int chunks, float* __restrict__ div) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  float mx = 0.f;
  for (int q = 0; q < chunks; ++q) mx = fmaxf(mx, part[(size_t)row * chunks + q]);
  div[row] = mx == 0.f ? 1.f : mx;
}

// the head through the top ReLU: S = [feat > 0] ? R / div : 0   (div == nullptr: no projection)
__global__ __launch_bounds__(256) void pattern_head_kernel(const f32x4* __restrict__ R, const f32x4* __restrict__ feat,
                                                           const int* __restrict__ row2img, const float* __restrict__ div,
                                                           f32x4* __restrict__ S, int n, size_t per4) {
  const size_t total = (size_t)n * per4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t t = i / per4, r = i - t * per4;
    const int img = row2img ? row2img[t] : (int)t;
    const f32x4 rv = R[i], fv = feat[(size_t)img * per4 + r];
    const float dv = div ? div[t] : 1.f;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fv[e] > 0.f ? (div ? rv[e] / dv : rv[e]) : 0.f;
    S[i] = o;
  }
}

struct PatternProjectArgs {
  const float* acc;      // (n, H, W, C) fp32: the transposed conv's plain accumulator = the tensor at the input of conv l
  const float* gate;     // (images, Hf, Wf, C): the forward's gate of the layer below; != 0 exactly at its live units (behind a
                         // pool: at the arg-max cell of a window, if that is live) — the mask [c > 0] and the pool's routing in one
  const int* row2img;
  const float* div;      // per row, or nullptr: no projection
  float* S;              // (n, Hf, Wf, C): what the next conv reads
  int n, H, W, C;
};
// An item is one pixel of conv l's input x 4 channels.  Behind a pool the projected tensor is routed first (its maximum stays 1:
// the pool-input tensor's projection is the identity) and then masked.
template <bool POOL>
__global__ __launch_bounds__(256) void pattern_project_kernel(PatternProjectArgs t) {
  const int cg = t.C / 4;
  const size_t HW = (size_t)t.H * t.W, per = HW * cg, total = (size_t)t.n * per;
  const int Hf = POOL ? 2 * t.H : t.H, Wf = POOL ? 2 * t.W : t.W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t row = i / per, rem = i - row * per, pix = rem / cg;
    const int c = (int)(rem - pix * cg) * 4;
    const int img = t.row2img ? t.row2img[row] : (int)row;
    f32x4 v = *reinterpret_cast<const f32x4*>(t.acc + (row * HW + pix) * t.C + c);
    if (t.div) {
      const float dv = t.div[row];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] / dv;
    }
    if constexpr (!POOL) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(t.gate + ((size_t)img * HW + pix) * t.C + c);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = v[e] * (g[e] != 0.f ? 1.f : 0.f);
      *reinterpret_cast<f32x4*>(t.S + (row * HW + pix) * t.C + c) = o;
    } else {
      const int y = (int)(pix / t.W), x = (int)(pix - (size_t)y * t.W);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const size_t cell = (size_t)(2 * y + (p >> 1)) * Wf + 2 * x + (p & 1);
        const f32x4 g = *reinterpret_cast<const f32x4*>(t.gate + ((size_t)img * Hf * Wf + cell) * t.C + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e] * (g[e] != 0.f ? 1.f : 0.f);
        *reinterpret_cast<f32x4*>(t.S + (row * (size_t)Hf * Wf + cell) * t.C + c) = o;
      }
    }
  }
}

// the image-level tensor, in place: x[row][:] /= div[row]
__global__ __launch_bounds__(256) void pattern_scale_kernel(float* __restrict__ x, size_t per_row, const float* __restrict__ div, int n) {
  if (!(per_row & 3)) {
    const size_t per4 = per_row / 4, total = (size_t)n * per4;
    f32x4* x4 = reinterpret_cast<f32x4*>(x);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
      const float dv = div[i / per4];
      f32x4 v = x4[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] / dv;
      x4[i] = v;
    }
  } else {
    const size_t total = (size_t)n * per_row;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) x[i] = x[i] / div[i / per_row];
  }
}

}  // namespace lrp
