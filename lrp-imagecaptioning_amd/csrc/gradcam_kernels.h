// gradcam_kernels.h — the Grad-CAM factor of the Guided Grad-CAM baselines (explainers.py:939-949 / :1643-1653, with the
// product of :934) and the map + statistic of the word examination (exaimin_word.py:95-102, :131-160, :488-489).  Two
// launches in the style of eval_kernels.h: one workgroup per unit / per map, fixed-order wave + LDS reductions, fp64
// accumulation, no float atomics: a unit's results do not depend on what else shares the launch.
//
//  gradcam_kernel    per unit u (image b = img_idx[u]), all in fp64 from the float32 inputs:
//      w_c = (1/L) sum_l grads[u][l][c];  A[l] = sum_c feat[b][l][c] w_c;  cam = M A M^T  (pyramid_expand, the matrix of
//      lrp_eval_expand_matrix);  cam = max(cam, 0);  cam /= max|cam| + 1e-6.  A cam that is nowhere positive is exact zeros.
//      Optional gate: out[u][p][c] = (double)gb[u][p][c] * cam[u][p] (numpy's float32 * float64 promotion, one multiply).
//      A unit whose image index lies outside [0, B) reads nothing and comes out as NaN.
//  exam_map_kernel   (n, H, W, C) relevance in T -> per pixel ((m[C-1] + m[C-2]) + ... + m[0]) / C in T (the rule of
//      eval_relevance_map_kernel without its sign / rectification), optional k x k block pooling to (H/k, W/k) in fp64
//      ('max' exact, 'ave' a row-major fp64 sum / k^2), x / absmax (all zeros when absmax == 0; no (x + 1) / 2 branch),
//      optional |x|; the map (T unpooled, fp64 pooled) and its fixed-order fp64 mean, each optional.
//      Nothing is staged: pass 2 recomputes what pass 1 reduced, so the kernel needs no scratch when the map is not wanted.
#pragma once
#include <hip/hip_runtime.h>
#include "eval_kernels.h"

namespace lrp {

constexpr int GRADCAM_MAX_D = 4096;   // channel weights share the LDS of the (g x S) intermediate

enum { EXAM_POOL_NONE = 0, EXAM_POOL_MAX = 1, EXAM_POOL_AVE = 2 };

// LDS: A (L) | U (max(D, g * S)): the channel weights until A is complete, then T[i][x] = sum_j A[i][j] M[x][j].
__global__ __launch_bounds__(256) void gradcam_kernel(const float* __restrict__ feat, const int* __restrict__ img_idx,
                                                      const float* __restrict__ grads, const double* __restrict__ M,
                                                      const float* __restrict__ gb, double* __restrict__ cams,
                                                      double* __restrict__ outs, int B, int g, int S, int D, int C) {
  extern __shared__ double lds[];
  const int L = g * g;
  double* A = lds;
  double* U = lds + L;
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t u = blockIdx.x;
  const int npix = S * S;
  double* o = cams + u * npix;
  const int b = img_idx[u];
  if (b < 0 || b >= B) {
    const double nan = 0.0 / 0.0;
    for (int p = tid; p < npix; p += 256) o[p] = nan;
    if (outs)
      for (size_t q = tid; q < (size_t)npix * C; q += 256) outs[u * npix * C + q] = nan;
    return;
  }
  const float* G = grads + u * L * D;
  const float* F = feat + (size_t)b * L * D;
  for (int c = tid; c < D; c += 256) {                      // channel weights: sequential over l, coalesced over c
    double s = 0.0;
    for (int l = 0; l < L; ++l) s += (double)G[(size_t)l * D + c];
    U[c] = s / (double)L;
  }
  __syncthreads();
  for (int l = wave; l < L; l += 4) {                       // A[l]: one wave per position, lanes stride the channels
    double s = 0.0;
    for (int c = lane; c < D; c += 64) s += (double)F[(size_t)l * D + c] * U[c];
    s = wave_sum_d(s);
    if (lane == 0) A[l] = s;
  }
  __syncthreads();                                          // U changes its meaning here
  for (int q = tid; q < g * S; q += 256) {
    const int i = q / S, x = q - i * S;
    double s = 0.0;
    for (int j = 0; j < g; ++j) s += A[i * g + j] * M[x * g + j];
    U[q] = s;
  }
  __syncthreads();
  double mx = 0.0;
  for (int p = tid; p < npix; p += 256) {
    const int y = p / S, x = p - y * S;
    double s = 0.0;
    for (int i = 0; i < g; ++i) s += M[y * g + i] * U[i * S + x];
    s = (s > 0.0 || s != s) ? s : 0.0;                      // np.maximum(cam, 0)
    o[p] = s;
    mx = s > mx ? s : mx;
  }
  mx = eval_wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  const double den = fmax(fmax(red[0], red[1]), fmax(red[2], red[3])) + 1e-6;
  for (int p = tid; p < npix; p += 256) {                   // same pixels per thread as the pass above
    const double v = o[p] / den;
    o[p] = v;
    if (outs) {
      const float* gp = gb + (u * npix + p) * C;
      double* op = outs + (u * npix + p) * C;
      for (int c = 0; c < C; ++c) op[c] = (double)gp[c] * v;
    }
  }
}

template <typename T>
__device__ __forceinline__ T exam_pixel_mean(const T* __restrict__ R, size_t p, int C) {
  T s = R[p * C + C - 1];
  for (int c = C - 2; c >= 0; --c) s = s + R[p * C + c];
  return s / (T)C;
}

// value of pooled cell (cy, cx): fp64 max (exact) or fp64 row-major mean of the k x k channel means
template <typename T>
__device__ __forceinline__ double exam_cell(const T* __restrict__ R, int W, int C, int k, int pool, int cy, int cx) {
  double acc = 0.0;
  for (int dy = 0; dy < k; ++dy)
    for (int dx = 0; dx < k; ++dx) {
      const double m = (double)exam_pixel_mean(R, (size_t)(cy * k + dy) * W + cx * k + dx, C);
      if (pool == EXAM_POOL_MAX) acc = (dy == 0 && dx == 0) ? m : (m > acc ? m : acc);
      else acc += m;
    }
  return pool == EXAM_POOL_MAX ? acc : acc / (double)(k * k);
}

template <typename T>
__global__ __launch_bounds__(256) void exam_map_kernel(const T* __restrict__ Rall, int H, int W, int C, int pool, int k,
                                                       int absval, void* __restrict__ maps, double* __restrict__ means) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t u = blockIdx.x;
  const T* R = Rall + u * H * W * C;
  double sum = 0.0;
  int cells;
  if (pool == EXAM_POOL_NONE) {
    cells = H * W;
    T mx = 0;
    for (int p = tid; p < cells; p += 256) {
      T m = exam_pixel_mean(R, p, C);
      m = m < T(0) ? -m : m;
      mx = m > mx ? m : mx;
    }
    mx = eval_wave_max(mx);
    if (lane == 0) red[wave] = (double)mx;
    __syncthreads();
    const T absmax = (T)fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));   // each red[] is a T value: exact both ways
    T* o = maps ? (T*)maps + u * cells : nullptr;
    for (int p = tid; p < cells; p += 256) {
      T v = absmax == T(0) ? T(0) : (T(1) * exam_pixel_mean(R, p, C)) / absmax;
      if (absval) v = (T)fabs((double)v);                     // np.abs: +0 for -0
      if (o) o[p] = v;
      sum += (double)v;
    }
  } else {
    const int ph = H / k, pw = W / k;
    cells = ph * pw;
    double mx = 0.0;
    for (int q = tid; q < cells; q += 256) {
      const double m = fabs(exam_cell(R, W, C, k, pool, q / pw, q % pw));
      mx = m > mx ? m : mx;
    }
    mx = eval_wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    const double absmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    double* o = maps ? (double*)maps + u * cells : nullptr;
    for (int q = tid; q < cells; q += 256) {
      double v = absmax == 0.0 ? 0.0 : (1.0 * exam_cell(R, W, C, k, pool, q / pw, q % pw)) / absmax;
      if (absval) v = fabs(v);
      if (o) o[q] = v;
      sum += v;
    }
  }
  if (!means) return;
  sum = wave_sum_d(sum);
  __syncthreads();                                          // red[] was read above
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) means[u] = (((red[0] + red[1]) + red[2]) + red[3]) / (double)cells;
}

}  // namespace lrp
