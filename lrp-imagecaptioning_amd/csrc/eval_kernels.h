// eval_kernels.h — bounding-box correctness evaluation (the reference's evaluate_bbox.py, EvaluationBboxCOCO /
// EvaluationBboxCOCOBaseline): per object word, the share of its normalised heat-map (and attention map) that lies inside
// the object's boxes, at several thresholds.  Three launches, one workgroup per map / per (map, box) entry, fixed-order
// wave + LDS reductions and no float atomics: a map's results do not depend on what else shares the launch.
//
//  eval_relevance_map_kernel  (n, npix, C) relevance -> (n, npix) map, same dtype, bit-identical to numpy's
//      hm = postprocess(R, 'BGRtoRGB'); hm = sign * hm; hm = max(hm, 0); hm = mean(hm, -1); hm = project(hm)
//      i.e. per pixel ((m[C-1] + m[C-2]) + ... + m[0]) / C in the flipped channel order, then x / absmax (all zeros when
//      absmax == 0).  Nothing here may be contracted or reassociated: the library is built without fast-math.
//  eval_attention_map_kernel  (n, g*g) float32 attention -> (n, S, S) float64: pyramid_expand(A) = M A M^T with the
//      (S x g) matrix M of the bilinear resize followed by the Gaussian blur (host-built), then project() including its
//      (x + 1) / 2 branch for maps with negative values.
//  eval_box_score_kernel      entries (map, y0, y1, x0, x1) x K thresholds -> (nb, K) float64
//      ratio_k = sum_box v [v > thr_k] / sum_all v [v > thr_k]  (0 when the denominator is 0, capped at 1).
//      The host encodes the reference's threshold carry-over in the per-entry thresholds.
#pragma once
#include <hip/hip_runtime.h>
#include "decoder_kernels.h"

namespace lrp {

constexpr int EVAL_MAX_K = 16;        // thresholds per box entry
constexpr int EVAL_MAX_G = 16;        // attention grid side
constexpr int EVAL_MAX_S = 448;       // expanded attention map side

template <typename T>
__device__ __forceinline__ T eval_pixel_mean(const T* __restrict__ R, size_t p, int C, T sign) {
  // numpy: (sign * flipped)[.., c] -> maximum(., 0) -> mean over the last axis (sequential adds, then / C)
  T s = 0;
  for (int c = C - 1; c >= 0; --c) {
    const T x = sign * R[p * C + c];
    const T m = (x > T(0) || x != x) ? x : T(0);          // np.maximum: +0 for -0, NaN propagates
    s = (c == C - 1) ? m : s + m;
  }
  return s / (T)C;
}

template <typename T>
__device__ __forceinline__ T eval_wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void eval_relevance_map_kernel(const T* __restrict__ Rall, T* __restrict__ maps, int npix,
                                                                 int C, T sign) {
  __shared__ T red[4];
  const T* R = Rall + (size_t)blockIdx.x * npix * C;
  T* o = maps + (size_t)blockIdx.x * npix;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T mx = 0;
  for (int p = tid; p < npix; p += 256) {                  // pass 1: channel mean (stored) and max |.| (values are >= 0)
    const T m = eval_pixel_mean(R, p, C, sign);
    o[p] = m;
    mx = m > mx ? m : mx;
  }
  mx = eval_wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  T absmax = red[0];
  for (int w = 1; w < 4; ++w) absmax = red[w] > absmax ? red[w] : absmax;
  for (int p = tid; p < npix; p += 256)                     // pass 2 (same pixels per thread as pass 1)
    o[p] = absmax == T(0) ? T(0) : (T(1) * o[p]) / absmax;
}

// T[i][x] = sum_j A[i][j] M[x][j] in LDS, then out[y][x] = sum_i M[y][i] T[i][x]; project() in two more passes.
__global__ __launch_bounds__(256) void eval_attention_map_kernel(const float* __restrict__ att, const double* __restrict__ M,
                                                                 double* __restrict__ maps, int g, int S) {
  extern __shared__ double lds[];
  double* A = lds;                        // g * g
  double* Tm = lds + g * g;               // g * S
  __shared__ double red[4];
  __shared__ int negs[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* a = att + (size_t)blockIdx.x * g * g;
  double* o = maps + (size_t)blockIdx.x * S * S;
  for (int i = tid; i < g * g; i += 256) A[i] = (double)a[i];
  __syncthreads();
  for (int q = tid; q < g * S; q += 256) {
    const int i = q / S, x = q - i * S;
    double s = 0.0;
    for (int j = 0; j < g; ++j) s += A[i * g + j] * M[x * g + j];
    Tm[q] = s;
  }
  __syncthreads();
  double mx = 0.0;
  for (int p = tid; p < S * S; p += 256) {
    const int y = p / S, x = p - y * S;
    double s = 0.0;
    for (int i = 0; i < g; ++i) s += M[y * g + i] * Tm[i * S + x];
    o[p] = s;
    mx = fmax(mx, fabs(s));
  }
  mx = eval_wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  const double absmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  int neg = 0;
  for (int p = tid; p < S * S; p += 256) {
    const double v = absmax == 0.0 ? 0.0 : (1.0 * o[p]) / absmax;
    o[p] = v;
    neg |= v < 0.0;
  }
  neg = __any(neg);
  if (lane == 0) negs[wave] = neg;
  __syncthreads();
  if (negs[0] | negs[1] | negs[2] | negs[3])
    for (int p = tid; p < S * S; p += 256) o[p] = (o[p] + 1.0) / 2.0;
}

// One workgroup per box entry: K totals over the whole map and K in-box sums over the box rows, fp64.  boxes (nb, 5) int32
// = (map, y0, y1, x0, x1) with 0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w (the host normalises Python slices); an entry that
// breaks this is not read and scores NaN.
template <typename T>
__global__ __launch_bounds__(256) void eval_box_score_kernel(const T* __restrict__ maps, int n, int h, int w,
                                                             const int* __restrict__ boxes, const double* __restrict__ thr,
                                                             int K, double* __restrict__ scores) {
  __shared__ double red[4][2 * EVAL_MAX_K];
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = boxes[e * 5], y0 = boxes[e * 5 + 1], y1 = boxes[e * 5 + 2], x0 = boxes[e * 5 + 3], x1 = boxes[e * 5 + 4];
  if (m < 0 || m >= n || y0 < 0 || y1 < y0 || y1 > h || x0 < 0 || x1 < x0 || x1 > w) {
    if (tid < K) scores[(size_t)e * K + tid] = 0.0 / 0.0;
    return;
  }
  const T* v = maps + (size_t)m * h * w;
  double th[EVAL_MAX_K], tot[EVAL_MAX_K], in[EVAL_MAX_K];
#pragma unroll
  for (int k = 0; k < EVAL_MAX_K; ++k) {
    th[k] = k < K ? thr[(size_t)e * K + k] : 0.0;
    tot[k] = 0.0;
    in[k] = 0.0;
  }
  const int npix = h * w;
  for (int p = tid; p < npix; p += 256) {
    const double x = (double)v[p];
#pragma unroll
    for (int k = 0; k < EVAL_MAX_K; ++k) tot[k] += x > th[k] ? x : 0.0;
  }
  const int bw = x1 - x0, nbox = (y1 - y0) * bw;
  for (int q = tid; q < nbox; q += 256) {
    const int y = y0 + q / bw, x = x0 + q % bw;
    const double u = (double)v[(size_t)y * w + x];
#pragma unroll
    for (int k = 0; k < EVAL_MAX_K; ++k) in[k] += u > th[k] ? u : 0.0;
  }
#pragma unroll
  for (int k = 0; k < EVAL_MAX_K; ++k) {
    if (k < K) {
      const double a = wave_sum_d(tot[k]), b = wave_sum_d(in[k]);
      if (lane == 0) { red[wave][k] = a; red[wave][EVAL_MAX_K + k] = b; }
    }
  }
  __syncthreads();
  if (tid < K) {
    const double t = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    const double c = ((red[0][EVAL_MAX_K + tid] + red[1][EVAL_MAX_K + tid]) + red[2][EVAL_MAX_K + tid]) + red[3][EVAL_MAX_K + tid];
    double r = t == 0.0 ? 0.0 : 1.0 * c / t;
    scores[(size_t)e * K + tid] = r > 1.0 ? 1.0 : r;
  }
}

}  // namespace lrp
